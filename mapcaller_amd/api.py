"""ctypes binding of include/mcx.h (libmcx.so) — the only way Python reaches the hot path.

There is no Python or CPU fallback: if libmcx.so is missing, or no GPU is visible when a device
function is called, an exception is raised.  torch tensors are accepted for device buffers only
as raw pointers (torch is plumbing for HBM allocation and torch.distributed).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCX_LIB") or os.path.join(_HERE, "libmcx.so")  # (MCX_LIB: another build of the same library, for experiments)
CIGAR_STRIDE = 32
CIGAR_SLACK = 65536


def cigar_pool_words(n_reads):
    """MCX_CIGAR_POOL_WORDS (include/mcx.h): the capacity of a batch's CIGAR pool."""
    return n_reads * CIGAR_STRIDE + CIGAR_SLACK


def pack_reads(bases, lens=None):
    """What mcx_stream_submit_packed takes, from ASCII reads: ``bases`` a torch uint8 tensor [n_reads, rlen] (any device; ``lens``
    optional int tensor of the reads' lengths).  Returns pinned host tensors (codes int32 [n_reads, row_words], len int32 [n_reads],
    odd int64 [n_odd]) — 2-bit codes sixteen bases to a word, first base on top; every byte that is not one of ACGT listed with its place."""
    import torch
    n, rlen = bases.shape
    row_words = (rlen + 15) // 16
    lut = torch.zeros(256, dtype=torch.int64, device=bases.device)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    known = torch.zeros(256, dtype=torch.bool, device=bases.device)
    for ch in b"ACGT":
        known[ch] = True
    b64 = bases.long()
    if lens is None:
        lens_t = torch.full((n,), rlen, dtype=torch.int64, device=bases.device)
    else:
        lens_t = lens.to(bases.device).long()
    inside = torch.arange(rlen, device=bases.device)[None, :] < lens_t[:, None]
    codes = lut[b64] * inside
    pad = row_words * 16 - rlen
    if pad:
        codes = torch.nn.functional.pad(codes, (0, pad))
    shifts = (30 - 2 * torch.arange(16, device=bases.device)).long()
    words = (codes.reshape(n, row_words, 16) << shifts).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    bad = (~known[b64]) & inside
    r, pos = torch.nonzero(bad, as_tuple=True)
    odd = (r << 32) | (pos << 8) | b64[r, pos]
    return (words.contiguous().cpu().pin_memory(), lens_t.to(torch.int32).cpu().pin_memory(), odd.cpu().pin_memory() if odd.numel() else torch.zeros(1, dtype=torch.int64).pin_memory(),
            int(odd.numel()), row_words)


# every symbol include/mcx.h declares
SYMBOLS = [
    "mcx_last_error", "mcx_device_count", "mcx_pack_row", "mcx_host_cpus", "mcx_gz_inflate", "mcx_index_load", "mcx_index_build", "mcx_index_from_codes", "mcx_index_save", "mcx_index_free", "mcx_index_trim",
    "mcx_index_genome_size", "mcx_index_n_chr", "mcx_index_chr_name", "mcx_index_chr_len", "mcx_index_hbm_bytes",
    "mcx_opts_default", "mcx_ctx_create", "mcx_ctx_create_fit", "mcx_ctx_free", "mcx_bwt_search_batch", "mcx_seed_walk_batch", "mcx_extend_batch", "mcx_extend_lanes",
    "mcx_avg_init", "mcx_map_batch_dev", "mcx_map_batch", "mcx_cigar_words", "mcx_map_files", "mcx_map_files_ex", "mcx_file_opts_default",
    "mcx_profile_attach", "mcx_profile_settle", "mcx_profile_finalize", "mcx_profile_sparse", "mcx_planes_alloc", "mcx_planes_free", "mcx_planes_bytes",
    "mcx_vcf_defaults", "mcx_call_variants", "mcx_vc_dense_dev",
    "mcx_batch_begin", "mcx_batch_sums", "mcx_batch_replay", "mcx_batch_end", "mcx_avg_walk", "mcx_batch_totals", "mcx_batch_check", "mcx_avg_advance", "mcx_exchange_local", "mcx_exchange_local_free",
    "mcx_profile_sparse_shard", "mcx_batch_end_keys", "mcx_batch_accumulate",
    "mcx_stream_submit", "mcx_stream_submit_packed", "mcx_stream_map", "mcx_stream_collect", "mcx_stream_next", "mcx_stream_mapped",
    "mcx_stream_map32", "mcx_stream_mapped32",
    "mcx_ctx_set_multi", "mcx_multi_lines", "mcx_multi_copy", "mcx_stream_multi",
    "mcx_sam_format_dev", "mcx_sam_format", "mcx_sam_header",
    "mcx_inflater_create", "mcx_inflater_free", "mcx_inflate_dev", "mcx_inflate", "mcx_bgzf_inflate",
    "mcx_gunzipper_create", "mcx_gunzipper_free", "mcx_gunzipper_reset", "mcx_gunzip_round_dev", "mcx_gunzip_text_dev", "mcx_gz_inflate_dev", "mcx_gz_inflate_dev_last",
    "mcx_fastq_parser_create", "mcx_fastq_parser_free", "mcx_fastq_parse_dev", "mcx_fastq_parse",
    "mcx_fastq_parser_set_rule", "mcx_stream_submit_dev", "mcx_files_route", "mcx_fastq_parser_set_format",
    "mcx_deflater_create", "mcx_deflater_free", "mcx_deflater_set_block", "mcx_bgzf_bound", "mcx_bgzf_deflate_dev", "mcx_bgzf_deflate", "mcx_bgzf_eof",
    "mcx_bam_format_dev", "mcx_bam_format", "mcx_bam_header", "mcx_bam_sort_dev", "mcx_bam_sort_last_ms", "mcx_bam_header_sorted", "mcx_files_sort_stats",
    "mcx_bam_index_dev", "mcx_bam_index_last_ms", "mcx_bgzf_deflate_blocks", "mcx_files_index_stats",
    "mcx_bam_dup_units_dev", "mcx_dup_resolve_dev", "mcx_bam_dup_mark_dev", "mcx_markdup_last_ms", "mcx_files_markdup_stats",
    "mcx_pass_last_shape",
    "mcx_md_dev", "mcx_md", "mcx_md_last_ms",
    "mcx_sam_format_tags_dev", "mcx_sam_format_tags", "mcx_bam_format_tags_dev", "mcx_bam_format_tags", "mcx_rg_parse", "mcx_sam_header_rg", "mcx_bam_header_rg", "mcx_map_files_rg",
    "mcx_bam_reads_header", "mcx_fastq_parser_set_reads", "mcx_fastq_parser_set_mates", "mcx_bam_reads_last", "mcx_bam_reads_last_ms",
]
# include/mcx_comm.h (libmcx_comm.so: the RCCL side, loaded by the native CLI only)
COMM_LIB_PATH = os.path.join(_HERE, "libmcx_comm.so")
COMM_SYMBOLS = ["mcx_comm_init_all", "mcx_comm_unique_id", "mcx_comm_init_rank", "mcx_comm_free", "mcx_comm_rank", "mcx_comm_size",
                "mcx_profile_reduce", "mcx_comm_exchange", "mcx_comm_exchange_free"]


class McxError(RuntimeError):
    pass


class Opts(C.Structure):
    _fields_ = [("alg", C.c_int32), ("max_pos_diff", C.c_int32), ("max_mismatch_rate", C.c_float),
                ("max_read_len", C.c_int32), ("max_batch_reads", C.c_int64)]


class Fit(C.Structure):  # mcx_fit
    _fields_ = [("pair_records_trimmed", C.c_int32), ("batch_halvings", C.c_int32), ("single_detail_set", C.c_int32), ("pad", C.c_int32),
                ("max_batch_reads", C.c_int64), ("hbm_free_bytes", C.c_int64), ("hbm_taken_bytes", C.c_int64)]


class Aln(C.Structure):
    _fields_ = [("pos", C.c_int64), ("mate_pos", C.c_int64), ("chr", C.c_int32), ("flag", C.c_int32),
                ("mapq", C.c_int32), ("tlen", C.c_int32), ("nm", C.c_int32), ("as_", C.c_int32), ("xs", C.c_int32),
                ("n_cigar", C.c_int32), ("fwd", C.c_int32), ("has_mate", C.c_int32), ("cigar_off", C.c_int32), ("pad", C.c_int32)]


ALN32_DTYPE = np.dtype([("pos_lo", "<u4"), ("mate_lo", "<u4"), ("pos_hi", "u1"), ("mate_hi", "u1"), ("mapq", "u1"), ("bits", "u1"), ("tlen", "<i4"), ("flag", "<u2"),
                        ("chr", "<u2"), ("nm", "<i2"), ("as", "<i2"), ("xs", "<i2"), ("n_cigar", "<u2"), ("cigar_off", "<u4")])  # mcx_aln32


def aln32_unpack(a32: np.ndarray) -> np.ndarray:
    """mcx_aln_unpack (include/mcx.h) over an array of mcx_aln32 records: the 64-byte form."""
    o = np.zeros(a32.shape, dtype=ALN_DTYPE)
    o["pos"] = a32["pos_lo"].astype(np.int64) | (a32["pos_hi"].astype(np.int64) << 32)
    o["mate_pos"] = a32["mate_lo"].astype(np.int64) | (a32["mate_hi"].astype(np.int64) << 32)
    o["chr"] = np.where(a32["chr"] == 0xFFFF, -1, a32["chr"].astype(np.int32))
    for f in ("flag", "mapq", "tlen", "nm", "as", "xs", "n_cigar", "cigar_off"):
        o[f] = a32[f]
    o["fwd"] = a32["bits"] & 1
    o["has_mate"] = (a32["bits"] >> 1) & 1
    return o


ALN_DTYPE = np.dtype([("pos", "<i8"), ("mate_pos", "<i8"), ("chr", "<i4"), ("flag", "<i4"), ("mapq", "<i4"),
                      ("tlen", "<i4"), ("nm", "<i4"), ("as", "<i4"), ("xs", "<i4"), ("n_cigar", "<i4"),
                      ("fwd", "<i4"), ("has_mate", "<i4"), ("cigar_off", "<i4"), ("pad", "<i4")])


# csrc/mcx_types.h DpSummary: what the lane that walked a DP problem's traceback leaves about its column string
DP_SUMMARY_DTYPE = np.dtype([("cols_off", "<u4"), ("cols_len", "<u2"), ("n", "<u2"), ("mis", "<u2"), ("switches", "<u2"), ("lead_d", "<u2"), ("lead_i", "<u2"),
                             ("lead_runs", "<u2"), ("tail_d", "<u2"), ("tail_i", "<u2"), ("tail_runs", "<u2"), ("n_rle", "<u2"), ("pad", "<u2"), ("rle", "<u4", (8,)),
                             ("pad2", "<u4")])
assert DP_SUMMARY_DTYPE.itemsize == 64


class SparseRec(C.Structure):
    _fields_ = [("pos", C.c_int64), ("type", C.c_uint8), ("len", C.c_uint8), ("seq", C.c_char * 54)]


PLANES = ("A", "C", "G", "T", "multi_hit", "readCount", "F1", "R2", "F2", "R1")


MULTI_PLANE = 4  # the one plane kept in 32 bits


def planes_stride(G: int) -> int:
    return (G + 63) & ~63


def planes_words(G: int) -> int:
    """32-bit words of the ten counter planes of a genome of G positions (mcx_planes_bytes / 4; csrc/mcx_planes.h): with
    stride = G rounded up to 64, multi_hit as u32 [stride], then A C G T readCount F1 R2 F2 R1 as u16 [stride] each."""
    return planes_stride(G) * 11 // 2


def planes_alloc(G: int, device):
    """Zeroed memory for the ten counter planes of a genome of G positions (what profile_attach takes): int32 [planes_words(G)]."""
    import torch
    return torch.zeros(planes_words(G), dtype=torch.int32, device=device)


def planes_parts(planes, G: int):
    """(multi_hit int32 [stride], the nine 16-bit planes int16 [9, stride] in the order A C G T readCount F1 R2 F2 R1): views."""
    import torch
    st = planes_stride(G)
    return planes[:st], planes[st:].view(torch.int16).reshape(9, st)


def planes_view(planes, G: int, lo: int = 0, hi: Optional[int] = None):
    """The positions [lo, hi) of all ten planes as int32 [10, hi - lo] in PLANES order (a copy)."""
    import torch
    hi = G if hi is None else hi
    multi, half = planes_parts(planes, G)
    out = torch.empty((10, hi - lo), dtype=torch.int32, device=planes.device)
    for k in range(10):
        if k == MULTI_PLANE:
            out[k] = multi[lo:hi]
        else:
            out[k] = half[k if k < MULTI_PLANE else k - 1, lo:hi].to(torch.int32) & 0xFFFF
    return out


def planes_from_rows(rows, device=None):
    """The planes' memory for counters given as int [10, G] in PLANES order (tests): the inverse of planes_view."""
    import torch
    G = rows.shape[1]
    planes = planes_alloc(G, device if device is not None else rows.device)
    multi, half = planes_parts(planes, G)
    multi[:G] = rows[MULTI_PLANE].to(torch.int32)
    for k in range(10):
        if k != MULTI_PLANE:
            v = rows[k].to(torch.int32) & 0xFFFF
            half[k if k < MULTI_PLANE else k - 1, :G] = torch.where(v >= 0x8000, v - 0x10000, v).to(torch.int16)
    return planes


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("reads", "mapped", "pairs", "pair_dist_sum", "pair_len_sum", "fm_ext_steps", "fm_blocks",
                                         "sa_hits", "dp_jobs", "dp_cells", "tier1_pairs", "replayed_pairs", "halved_selections", "simple_pairs")] + \
               [(n, C.c_double) for n in ("ms_encode", "ms_seed", "ms_sa", "ms_cluster", "ms_rescue", "ms_build",
                                          "ms_dp", "ms_finish", "ms_total", "ms_simple", "ms_order")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)


class Exchange(C.Structure):
    """mcx_exchange: the collective the shards of one run share (all-gather of host bytes)."""
    _fields_ = [("user", C.c_void_p), ("rank", C.c_int32), ("size", C.c_int32), ("allgather", ALLGATHER)]


def dist_exchange(device=None) -> Exchange:
    """An mcx_exchange over torch.distributed (backend "nccl" = RCCL: staged through ``device``;
    "gloo": host tensors).  Keep the returned object alive while the run uses it."""
    import torch
    import torch.distributed as dist
    world, rank = dist.get_world_size(), dist.get_rank()
    on_gpu = dist.get_backend() == "nccl"

    def allgather(user, send, recv, nbytes):
        try:
            if nbytes == 0:
                return 0
            mine = torch.frombuffer((C.c_uint8 * nbytes).from_address(send), dtype=torch.uint8).clone()
            if on_gpu:
                mine = mine.to(device)
            parts = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            out = torch.cat(parts).cpu().contiguous()
            C.memmove(recv, out.data_ptr(), world * nbytes)
            return 0
        except Exception as e:  # the C side turns this into an error on every shard
            import sys
            print(f"mcx exchange: {e}", file=sys.stderr)
            return -3

    x = Exchange()
    x.user, x.rank, x.size = None, rank, world
    x.allgather = ALLGATHER(allgather)
    return x


class FileOpts(C.Structure):
    """mcx_file_opts: -p, -t, library append, -gpu_sam, insert-size state across libraries, sharding, -gpu_inflate, -gpu_parse."""
    _fields_ = [("interleaved_pairs", C.c_int32), ("host_threads", C.c_int32), ("append_sam", C.c_int32), ("device_sam", C.c_int32),
                ("avg_state", C.POINTER(C.c_int64)), ("shard_rank", C.c_int32), ("shard_count", C.c_int32), ("device_inflate", C.c_int32), ("device_parse", C.c_int32),
                ("exchange", C.POINTER(Exchange))]


class SamIn(C.Structure):
    """mcx_sam_in: what mcx_sam_format[_dev] makes a batch's SAM text from (pointers as integers: host or device)."""
    _fields_ = [(n, C.c_void_p) for n in ("bases", "off", "qual", "names", "name_off", "aln", "cigar", "x_index", "x_recs", "x_cigar")] + \
               [("n_reads", C.c_uint32), ("paired", C.c_int32), ("md", C.c_void_p), ("md_off", C.c_void_p)]  # (md / md_off: mcx_md[_dev]'s strings; null: no MD:Z tag)


class SamTags(C.Structure):
    """mcx_sam_tags: what travels beside mcx_sam_in for -rg / -mc — the read group's ID (host or device bytes; null: no RG:Z) and the MC:Z / MQ:i switch"""
    _fields_ = [("rg", C.c_void_p), ("rg_len", C.c_uint32), ("mate_tags", C.c_int32)]


ERR_IO, ERR_ARG = -1, -2  # MCX_ERR_IO, MCX_ERR_ARG
ERR_CAPACITY = -4  # MCX_ERR_CAPACITY
# mcx_deflate_member: one BGZF member's raw deflate stream src[src_off:][:src_len] -> dst[dst_off:][:isize], with the CRC-32 of its text
MEMBER_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("src_len", "<u4"), ("isize", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])
# mcx_fastq_rec: one FASTQ record as offsets into its own text; mcx_fastq_stop
FASTQ_RULE_PLAIN, FASTQ_RULE_GZ = 0, 1  # mcx_fastq_rule
READS_FASTQ, READS_FASTA = 0, 1  # mcx_reads_format
READS_BAM = 2  # mcx_reads_format_bam: BAM records, found and unpacked on the device
ROUTE_BAM_IN = 1024  # the read file is BAM
ROUTE_INFLATE, ROUTE_PARSE, ROUTE_ROWS, ROUTE_SAM = 1, 2, 4, 8  # mcx_route
ROUTE_BGZF = 16
ROUTE_BAM = 32
ROUTE_SORT = 64
ROUTE_INDEX = 128
ROUTE_MARKDUP = 256
ROUTE_GZ = 512  # the file's ordinary gzip stream was inflated on the device
INFLATE_BGZF, INFLATE_GZ = 1, 2  # bits of mcx_file_opts.device_inflate
GZ_OK, GZ_DAMAGED, GZ_INPUT, GZ_CAPACITY, GZ_MORE = 0, 1, 2, 3, 4  # mcx_gz_status


class GzRound(C.Structure):
    """mcx_gz_round: what a round of a Gunzipper did."""
    _fields_ = [("end_bit", C.c_uint64), ("text_bytes", C.c_uint64), ("crc32", C.c_uint32), ("final", C.c_uint32), ("status", C.c_uint32),
                ("stretches", C.c_uint32), ("starts", C.c_uint32), ("chain", C.c_uint32), ("overflowed", C.c_uint32), ("ms", C.c_float * 4)]
SAM_MARKDUP = 32  # (mcx_sam_bits, below)
DUP_NONE, DUP_FRAGMENT, DUP_PAIR, DUP_SECOND_MATE = 0, 1, 2, 4  # mcx_dup_unit.kind: bits 0-1 the kind, bit 2 a paired input's fragment is the second read
DUP_UNIT_DTYPE = np.dtype([("end0", "<u8"), ("end1", "<u8"), ("score", "<u4"), ("kind", "<u4")])  # mcx_dup_unit, 24 bytes
SAM_INDEX = 16  # (mcx_sam_bits, below)
SAM_MD = 64  # (mcx_sam_bits: an MD:Z tag on every mapped line; with the host formatter too)
SAM_MC = 128  # (mcx_sam_bits: MC:Z and MQ:i on the lines of pairs; with the host formatter too)
ERR_UNSUPPORTED = -5  # MCX_ERR_UNSUPPORTED
SAM_DEVICE, SAM_BGZF, SAM_BAM, SAM_SORT = 1, 2, 4, 8  # mcx_sam_bits (mcx_file_opts.device_sam); SAM_INDEX = 16 above
BGZF_BLOCK = 65280  # bytes of text per BGZF block: bgzip's cut
REC_DTYPE = np.dtype([("name", "<u4"), ("name_len", "<u4"), ("seq", "<u4"), ("rlen", "<u4"), ("qual", "<u4"), ("q_take", "<u4")])
FASTQ_MORE, FASTQ_END, FASTQ_EMPTY, FASTQ_TOO_LONG = 0, 1, 2, 3
FASTQ_DAMAGED, FASTQ_UNPAIRED = 4, 5  # mcx_fastq_stop_bam: under READS_BAM alone


class BaiRun(C.Structure):
    """mcx_bai_run: a stretch of records with one (contig, bin) — the virtual offset of its first record and its records without / with flag bit 4"""
    _fields_ = [("ref_id", C.c_int32), ("bin", C.c_uint32), ("u", C.c_uint64), ("n_mapped", C.c_uint32), ("n_unmapped", C.c_uint32)]


BAI_RUN_DTYPE = np.dtype([("ref_id", "<i4"), ("bin", "<u4"), ("u", "<u8"), ("n_mapped", "<u4"), ("n_unmapped", "<u4")])


class FastqIn(C.Structure):
    """mcx_fastq_in (pointers as integers: host or device)"""
    _fields_ = [("text", C.c_void_p * 2), ("bytes", C.c_uint64 * 2), ("max_records", C.c_uint32), ("max_read_len", C.c_int32), ("final", C.c_int32), ("n_ref", C.c_int32)]


class FastqOut(C.Structure):
    """mcx_fastq_out (pointers as integers: host or device)"""
    _fields_ = [("recs", C.c_void_p * 2), ("bases", C.c_void_p), ("off", C.c_void_p), ("qual", C.c_void_p), ("bases_cap", C.c_uint64),
                ("names", C.c_void_p), ("name_off", C.c_void_p), ("names_cap", C.c_uint64),
                ("rows", C.c_void_p), ("row_words", C.c_uint32), ("len", C.c_void_p), ("odd", C.c_void_p), ("odd_cap", C.c_uint32)]


class FastqInfo(C.Structure):
    """mcx_fastq_info"""
    _fields_ = [("n_records", C.c_uint32 * 2), ("stop", C.c_uint32 * 2), ("consumed", C.c_uint64 * 2), ("n_reads", C.c_uint32), ("longest", C.c_uint32),
                ("n_odd", C.c_uint32), ("pad", C.c_uint32), ("n_bases", C.c_uint64), ("n_name_bytes", C.c_uint64)]

    def as_dict(self) -> dict:
        return {"n_records": list(self.n_records), "stop": list(self.stop), "consumed": list(self.consumed), "n_reads": self.n_reads, "longest": self.longest,
                "n_odd": self.n_odd, "n_bases": self.n_bases, "n_name_bytes": self.n_name_bytes}


class VcfOpts(C.Structure):
    """mcx_vcf_opts: MapCaller's variant-calling switches (reference src/main.cpp:157-187)."""
    _fields_ = [(n, C.c_int32) for n in ("ploidy", "min_allele_depth", "min_cnv", "min_gap", "fragment_size", "filter", "gvcf",
                                         "monomorphic", "somatic", "max_dup", "max_clip")] + \
               [("freq_thr", C.c_float), ("sample_id", C.c_char_p), ("ref_name", C.c_char_p), ("cmdline", C.c_char_p)]


class VcfStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_snv", "n_ins", "n_del", "n_inv", "n_tnl", "n_records")] + \
               [("avg_read_len", C.c_int32), ("fragment_size", C.c_int32)] + \
               [(n, C.c_double) for n in ("ms_depth", "ms_scan", "ms_total")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# the records of mcx_vc_dense_dev (csrc/mcx_variants_host.h SiteRec, Column, RangeQ)
VC_SITE_DTYPE = np.dtype([("pos", "<i8"), ("type", "u1"), ("geno", "u1"), ("qscore", "u1"), ("alt", "u1"), ("DP", "<u2"), ("AD_ref", "<u2"),
                          ("AD_alt", "<u2"), ("pad", "<u2"), ("pad2", "<u4")])
VC_COLUMN_DTYPE = np.dtype([("v", "<u4", (10,)), ("depth", "<i4"), ("ref", "<u4")])
VC_RANGE_DTYPE = np.dtype([("beg", "<i8"), ("end", "<i8"), ("mode", "<i4"), ("pad", "<i4")])
assert (VC_SITE_DTYPE.itemsize, VC_COLUMN_DTYPE.itemsize, VC_RANGE_DTYPE.itemsize) == (24, 48, 24)


def vcf_opts(**switches):
    """mcx_vcf_opts at the reference's defaults with ``switches`` (its fields) set; strings are kept alive by the second value."""
    o = VcfOpts()
    lib().mcx_vcf_defaults(C.byref(o))
    keep = []
    for k, v in switches.items():
        if isinstance(v, str):
            v = v.encode()
            keep.append(v)
        setattr(o, k, v)
    return o, keep


def vc_dense(d_pac_ptr: int, G: int, d_planes_ptr: int, positions=(), ranges=(), device: int = 0, **switches):
    """mcx_vc_dense_dev (tests): the variant caller's dense half over planes and a packed genome in HBM.  ``positions``: genome
    positions; ``ranges``: (beg, end, mode) rows, mode 0 coverage sum, 1 minimum over covered positions.  Returns (the ordered
    records as VC_SITE_DTYPE, the columns as VC_COLUMN_DTYPE, the range values as uint64), each a numpy array of its own."""
    o, _keep = vcf_opts(**switches)
    pos = np.ascontiguousarray(positions, dtype=np.int64).reshape(-1)
    rq = np.zeros(len(ranges), dtype=VC_RANGE_DTYPE)
    if len(ranges):
        r = np.asarray(ranges, dtype=np.int64).reshape(-1, 3)
        rq["beg"], rq["end"], rq["mode"] = r[:, 0], r[:, 1], r[:, 2]
    cols = np.zeros(len(pos), dtype=VC_COLUMN_DTYPE)
    vals = np.zeros(len(rq), dtype=np.uint64)
    p_sites, n_sites = C.c_void_p(), C.c_uint64()
    _check(lib().mcx_vc_dense_dev(device, d_pac_ptr, G, d_planes_ptr, C.byref(o), pos.ctypes.data, len(pos), rq.ctypes.data, len(rq),
                                  C.byref(p_sites), C.byref(n_sites), cols.ctypes.data, vals.ctypes.data), "mcx_vc_dense_dev")
    n = int(n_sites.value)
    sites = np.empty(n, dtype=VC_SITE_DTYPE)
    if n:
        C.memmove(sites.ctypes.data, p_sites.value, n * VC_SITE_DTYPE.itemsize)
    return sites, cols, vals


_lib = None


def lib() -> C.CDLL:
    """Loads libmcx.so (built by ``make -C mapcaller_amd/csrc`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.environ.get("MCX_NO_TORCH"):  # (a host without torch in it — mapcaller_amd/boundary.py — runs on the system's runtime, which libmcx.so links)
        try:  # torch bundles its own HIP runtime: let it load first so that both share one copy
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(LIB_PATH):
        raise McxError(f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')")
    L = C.CDLL(LIB_PATH)
    L.mcx_last_error.restype = C.c_char_p
    L.mcx_index_genome_size.restype = C.c_int64
    L.mcx_index_hbm_bytes.restype = C.c_int64
    L.mcx_index_chr_name.restype = C.c_char_p
    L.mcx_index_load.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.mcx_index_build.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.mcx_index_from_codes.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p), C.POINTER(C.c_double)]
    L.mcx_index_save.argtypes = [C.c_void_p, C.c_char_p]
    L.mcx_index_trim.argtypes = [C.c_void_p, C.c_int]
    for f in (L.mcx_index_free, L.mcx_ctx_free):
        f.argtypes = [C.c_void_p]
        f.restype = None
    for f in (L.mcx_index_genome_size, L.mcx_index_n_chr, L.mcx_index_hbm_bytes):
        f.argtypes = [C.c_void_p]
    L.mcx_index_chr_name.argtypes = [C.c_void_p, C.c_int32]
    L.mcx_index_chr_len.argtypes = [C.c_void_p, C.c_int32]
    L.mcx_opts_default.argtypes = [C.POINTER(Opts)]
    L.mcx_opts_default.restype = None
    L.mcx_ctx_create.argtypes = [C.c_void_p, C.POINTER(Opts), C.POINTER(C.c_void_p)]
    L.mcx_ctx_create_fit.argtypes = [C.c_void_p, C.POINTER(Opts), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(Fit)]
    L.mcx_bwt_search_batch.argtypes = [C.c_void_p] + [C.c_void_p] * 3 + [C.c_uint32] + [C.c_void_p] * 3
    L.mcx_seed_walk_batch.argtypes = [C.c_void_p] + [C.c_void_p] * 2 + [C.c_uint32, C.c_int, C.c_uint32] + [C.c_void_p] * 2
    L.mcx_extend_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 3
    L.mcx_extend_lanes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 4
    L.mcx_avg_init.argtypes = [C.POINTER(C.c_int64)]
    L.mcx_avg_init.restype = None
    for f in (L.mcx_map_batch_dev, L.mcx_map_batch):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_int64), C.c_void_p,
                      C.c_void_p, C.POINTER(Stats)]
    L.mcx_map_files.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(Stats)]
    L.mcx_map_files_ex.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(FileOpts), C.c_char_p, C.POINTER(Stats)]
    L.mcx_file_opts_default.argtypes = [C.POINTER(FileOpts)]
    L.mcx_file_opts_default.restype = None
    L.mcx_profile_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.mcx_profile_settle.argtypes = [C.c_void_p]
    L.mcx_profile_finalize.argtypes = [C.c_void_p, C.c_void_p]
    L.mcx_profile_sparse.argtypes = [C.c_void_p, C.POINTER(C.POINTER(SparseRec)), C.POINTER(C.c_uint64)]
    L.mcx_profile_sparse_shard.argtypes = [C.c_void_p, C.POINTER(C.POINTER(SparseRec)), C.POINTER(C.c_uint64)]
    L.mcx_batch_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    L.mcx_batch_sums.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)] + [C.POINTER(C.POINTER(C.c_uint32))] * 3
    L.mcx_batch_replay.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(Stats)]
    L.mcx_batch_end.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.mcx_batch_end_keys.argtypes = [C.c_void_p, C.POINTER(Stats), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]
    L.mcx_batch_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]
    L.mcx_avg_walk.argtypes = [C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.mcx_avg_walk.restype = None
    L.mcx_batch_totals.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.mcx_batch_check.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_uint32), C.POINTER(Stats)]
    L.mcx_avg_advance.argtypes = [C.POINTER(C.c_int64), C.c_int64, C.c_int64, C.c_int64]
    L.mcx_avg_advance.restype = None
    L.mcx_exchange_local.argtypes = [C.c_int32, C.POINTER(Exchange)]
    L.mcx_exchange_local_free.argtypes = [C.POINTER(Exchange)]
    L.mcx_exchange_local_free.restype = None
    L.mcx_stream_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.mcx_stream_submit_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.mcx_stream_submit_dev.restype = C.c_int
    L.mcx_stream_submit_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.mcx_files_route.restype = C.c_int
    L.mcx_files_route.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.mcx_fastq_parser_set_rule.restype = C.c_int
    L.mcx_fastq_parser_set_rule.argtypes = [C.c_void_p, C.c_int]
    L.mcx_fastq_parser_set_format.restype = C.c_int
    L.mcx_fastq_parser_set_format.argtypes = [C.c_void_p, C.c_int]
    L.mcx_fastq_parser_set_reads.restype = C.c_int
    L.mcx_fastq_parser_set_reads.argtypes = [C.c_void_p, C.c_int]
    L.mcx_fastq_parser_set_mates.restype = C.c_int
    L.mcx_fastq_parser_set_mates.argtypes = [C.c_void_p, C.c_int]
    L.mcx_bam_reads_last.restype = C.c_int
    L.mcx_bam_reads_last.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mcx_bam_reads_last_ms.restype = C.c_int
    L.mcx_bam_reads_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mcx_bam_reads_header.restype = C.c_int
    L.mcx_bam_reads_header.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    L.mcx_stream_map.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    L.mcx_stream_map32.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    L.mcx_stream_mapped32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mcx_stream_collect.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mcx_ctx_set_multi.argtypes = [C.c_void_p, C.c_int, C.c_uint32]
    L.mcx_multi_lines.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_uint32)] * 2
    L.mcx_multi_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mcx_stream_multi.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 3 + [C.POINTER(C.c_uint32)] * 3
    L.mcx_planes_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.mcx_planes_free.argtypes = [C.c_void_p]
    L.mcx_planes_free.restype = None
    L.mcx_planes_bytes.argtypes = [C.c_int64]
    L.mcx_planes_bytes.restype = C.c_uint64
    L.mcx_vcf_defaults.argtypes = [C.POINTER(VcfOpts)]
    L.mcx_vcf_defaults.restype = None
    L.mcx_call_variants.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_int64,
                                    C.POINTER(VcfOpts), C.c_char_p, C.POINTER(VcfStats)]
    L.mcx_vc_dense_dev.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(VcfOpts), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                   C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
    L.mcx_gz_inflate.restype = C.c_int64
    L.mcx_gz_inflate.argtypes = [C.c_char_p, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    for f in (L.mcx_sam_format_dev, L.mcx_sam_format):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SamIn), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
    L.mcx_sam_header.restype = C.c_int
    L.mcx_sam_header.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    for f in (L.mcx_bam_format_dev, L.mcx_bam_format):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SamIn), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mcx_bam_header.restype = C.c_int
    L.mcx_bam_header.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_bam_sort_dev.restype = C.c_int
    L.mcx_bam_sort_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.mcx_bam_sort_last_ms.restype = C.c_int
    L.mcx_bam_sort_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mcx_pass_last_shape.restype = C.c_int
    L.mcx_pass_last_shape.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.mcx_bam_header_sorted.restype = C.c_int
    L.mcx_bam_header_sorted.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_files_sort_stats.restype = C.c_int
    L.mcx_files_sort_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mcx_bam_index_dev.restype = C.c_int
    L.mcx_bam_index_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                    C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_bam_index_last_ms.restype = C.c_int
    L.mcx_bam_index_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mcx_bam_dup_units_dev.restype = C.c_int
    L.mcx_bam_dup_units_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
    L.mcx_dup_resolve_dev.restype = C.c_int
    L.mcx_dup_resolve_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.mcx_bam_dup_mark_dev.restype = C.c_int
    L.mcx_bam_dup_mark_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
    L.mcx_markdup_last_ms.restype = C.c_int
    L.mcx_markdup_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mcx_files_markdup_stats.restype = C.c_int
    L.mcx_files_markdup_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mcx_files_index_stats.restype = C.c_int
    L.mcx_files_index_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mcx_bgzf_deflate_blocks.restype = C.c_int
    L.mcx_bgzf_deflate_blocks.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    for f in (L.mcx_md_dev, L.mcx_md):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SamIn), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
    for f in (L.mcx_sam_format_tags_dev, L.mcx_sam_format_tags):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SamIn), C.POINTER(SamTags), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
    for f in (L.mcx_bam_format_tags_dev, L.mcx_bam_format_tags):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(SamIn), C.POINTER(SamTags), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mcx_rg_parse.restype = C.c_int
    L.mcx_rg_parse.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.mcx_sam_header_rg.restype = C.c_int
    L.mcx_sam_header_rg.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_bam_header_rg.restype = C.c_int
    L.mcx_bam_header_rg.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_map_files_rg.restype = C.c_int
    L.mcx_map_files_rg.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(FileOpts), C.c_char_p, C.c_char_p, C.POINTER(Stats)]
    L.mcx_md_last_ms.restype = C.c_int
    L.mcx_md_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mcx_bam_last_ms.restype = C.c_int
    L.mcx_bam_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mcx_inflater_create.restype = C.c_int
    L.mcx_inflater_create.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.mcx_inflater_free.restype = None
    L.mcx_inflater_free.argtypes = [C.c_void_p]
    for f in (L.mcx_inflate_dev, L.mcx_inflate):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    L.mcx_fastq_parser_create.restype = C.c_int
    L.mcx_fastq_parser_create.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    L.mcx_fastq_parser_free.restype = None
    L.mcx_fastq_parser_free.argtypes = [C.c_void_p]
    for f in (L.mcx_fastq_parse_dev, L.mcx_fastq_parse):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.POINTER(FastqIn), C.POINTER(FastqOut), C.POINTER(FastqInfo)]
    L.mcx_fastq_last_ms.restype = C.c_int
    L.mcx_fastq_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mcx_fastq_grown.restype = C.c_int
    L.mcx_fastq_grown.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.mcx_inflate_last_ms.restype = C.c_int
    L.mcx_inflate_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mcx_bgzf_inflate.restype = C.c_int64
    L.mcx_bgzf_inflate.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_gunzipper_create.restype = C.c_int
    L.mcx_gunzipper_create.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_void_p)]
    L.mcx_gunzipper_free.restype = None
    L.mcx_gunzipper_free.argtypes = [C.c_void_p]
    L.mcx_gunzipper_reset.restype = None
    L.mcx_gunzipper_reset.argtypes = [C.c_void_p]
    L.mcx_gunzip_round_dev.restype = C.c_int
    L.mcx_gunzip_round_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(GzRound)]
    L.mcx_gunzip_text_dev.restype = C.c_int
    L.mcx_gunzip_text_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(GzRound)]
    L.mcx_gz_inflate_dev.restype = C.c_int64
    L.mcx_gz_inflate_dev.argtypes = [C.c_char_p, C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_gz_inflate_dev_last.restype = None
    L.mcx_gz_inflate_dev_last.argtypes = [C.POINTER(C.c_uint64 * 2)]
    L.mcx_deflater_create.restype = C.c_int
    L.mcx_deflater_create.argtypes = [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]
    L.mcx_deflater_free.restype = None
    L.mcx_deflater_free.argtypes = [C.c_void_p]
    L.mcx_deflater_set_block.restype = C.c_int
    L.mcx_deflater_set_block.argtypes = [C.c_void_p, C.c_uint32]
    L.mcx_bgzf_bound.restype = C.c_uint64
    L.mcx_bgzf_bound.argtypes = [C.c_uint64, C.c_uint32]
    for f in (L.mcx_bgzf_deflate_dev, L.mcx_bgzf_deflate):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mcx_bgzf_eof.restype = C.c_int
    L.mcx_bgzf_eof.argtypes = [C.c_void_p]
    L.mcx_bgzf_deflate_last_ms.restype = C.c_int
    L.mcx_bgzf_deflate_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc != 0:
        raise McxError(f"{what} failed ({rc}): {lib().mcx_last_error().decode()}")


def device_count() -> int:
    return int(lib().mcx_device_count())


class Index:
    """FM-index + reference resident in HBM (mcx_index_load; reference src/bwt_index.cpp:150-258)."""

    def __init__(self, prefix: Optional[str], device: int = 0, full_sa: int = 0):
        # full_sa: 0 the sampled suffix array as on disk; 1 (True) every entry + jump table + rank records; 2 + the pair records
        self._h = C.c_void_p()
        self.device = device
        self.build_seconds = None
        if prefix is not None:
            _check(lib().mcx_index_load(prefix.encode(), device, int(full_sa), C.byref(self._h)), "mcx_index_load")

    @classmethod
    def from_codes(cls, d_codes_ptr: int, chr_lens: List[int], chr_names: Optional[List[str]] = None, device: int = 0,
                   full_sa: int = 0) -> "Index":
        """Builds the index on the GPU from a genome already in HBM (codes 0..3, contigs concatenated)."""
        self = cls(None, device)
        n = len(chr_lens)
        lens = (C.c_int32 * n)(*chr_lens)
        names = (C.c_char_p * n)(*[(chr_names[i] if chr_names else f"chr{i + 1}").encode() for i in range(n)])
        secs = C.c_double()
        _check(lib().mcx_index_from_codes(d_codes_ptr, n, lens, names, device, int(full_sa), C.byref(self._h), C.byref(secs)),
               "mcx_index_from_codes")
        self.build_seconds = secs.value
        return self

    def save(self, prefix: str) -> None:
        _check(lib().mcx_index_save(self._h, prefix.encode()), "mcx_index_save")

    def trim(self, full_sa: int = 1) -> None:
        """Gives back what the index holds above the level ``full_sa`` (1: the pair records of full_sa=2).  Mappers made
        before must have been closed."""
        _check(lib().mcx_index_trim(self._h, int(full_sa)), "mcx_index_trim")

    @staticmethod
    def build(fasta: str, prefix: str, device: int = 0) -> None:
        _check(lib().mcx_index_build(fasta.encode(), prefix.encode(), device), "mcx_index_build")

    @property
    def genome_size(self) -> int:
        return int(lib().mcx_index_genome_size(self._h))

    @property
    def hbm_bytes(self) -> int:
        return int(lib().mcx_index_hbm_bytes(self._h))

    @property
    def chromosomes(self) -> List[Tuple[str, int]]:
        L = lib()
        return [(L.mcx_index_chr_name(self._h, i).decode(), int(L.mcx_index_chr_len(self._h, i)))
                for i in range(L.mcx_index_n_chr(self._h))]

    def call_variants(self, d_planes_ptr: int, sparse, pairs: int, pair_dist_sum: int, pair_len_sum: int, vcf_path: str,
                      **switches) -> dict:
        """VariantCalling() over finalized planes (reference src/VariantCalling.cpp:696-740).
        ``sparse``: the records of Mapper.profile_sparse() (of all ranks); ``pairs`` /
        ``pair_dist_sum`` / ``pair_len_sum``: totals of Mapper.stats.  ``switches``: fields of
        mcx_vcf_opts (ploidy, min_allele_depth, min_cnv, min_gap, fragment_size, filter, gvcf,
        monomorphic, somatic, sample_id, ref_name, cmdline)."""
        o, _keep = vcf_opts(**switches)
        if isinstance(sparse, np.ndarray):  # raw mcx_sparse_rec bytes
            raw = np.ascontiguousarray(sparse, dtype=np.uint8).reshape(-1, 64)
            st = VcfStats()
            _check(lib().mcx_call_variants(self._h, d_planes_ptr, raw.ctypes.data, raw.shape[0], pairs, pair_dist_sum, pair_len_sum, C.byref(o),
                                           vcf_path.encode(), C.byref(st)), "mcx_call_variants")
            return st.as_dict()
        rows = []  # (type, pos, len byte, payload); a string longer than a record continues in 'C' records behind it
        for t, pos, x in sparse:
            if t in "VT":
                rows.append((t, pos, 0, int(x).to_bytes(8, "little", signed=True)))
            else:
                b = x.encode("latin-1")
                rows.append((t, pos, min(len(b), 255), b[:54]))
                for lo in range(54, len(b), 54):
                    rows.append(("C", pos, len(b[lo:lo + 54]), b[lo:lo + 54]))
        recs = (SparseRec * max(len(rows), 1))()
        for i, (t, pos, ln, payload) in enumerate(rows):
            r = recs[i]
            r.pos, r.type, r.len = pos, ord(t), ln
            C.memmove(C.addressof(r) + 10, payload, len(payload))
        st = VcfStats()
        _check(lib().mcx_call_variants(self._h, d_planes_ptr, recs, len(rows), pairs, pair_dist_sum, pair_len_sum, C.byref(o),
                                       vcf_path.encode(), C.byref(st)), "mcx_call_variants")
        return st.as_dict()

    def close(self):
        if self._h:
            lib().mcx_index_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mapper:
    """One mapping context (mcx_ctx): a GPU, its scratch and the reference's tunables."""

    def __init__(self, index: Index, alg: str = "nw", max_read_len: int = 256, max_batch_reads: int = 1 << 20,
                 max_pos_diff: int = 30, max_mismatch_rate: float = 0.05, multi: bool = False, multi_cap: int = 0):
        """``multi``: -m — a SAM line for every candidate with a read's best score (map_batch returns them as a third element, map_files
        writes them behind the read's first line); ``multi_cap``: the initial capacity of the extras pool in lines (0: a default; it grows)."""
        if alg not in ("nw", "ksw2"):
            raise ValueError("alg must be 'nw' or 'ksw2'")
        self.index = index
        self.multi = bool(multi)
        self.stream_multi = []  # (multi) map_stream*: every collected batch's extras, in input order (stream_multi_collected)
        o = Opts()
        lib().mcx_opts_default(C.byref(o))
        o.alg = 0 if alg == "nw" else 1
        o.max_read_len = max_read_len
        o.max_batch_reads = max_batch_reads
        o.max_pos_diff = max_pos_diff
        o.max_mismatch_rate = max_mismatch_rate
        self._h = C.c_void_p()
        _check(lib().mcx_ctx_create(index._h, C.byref(o), C.byref(self._h)), "mcx_ctx_create")
        if self.multi:
            _check(lib().mcx_ctx_set_multi(self._h, 1, int(multi_cap)), "mcx_ctx_set_multi")
        self.avg = (C.c_int64 * 4)()
        lib().mcx_avg_init(self.avg)
        self.stats = Stats()

    @staticmethod
    def fit_plan(index: Index, alg: str = "nw", max_read_len: int = 256, max_batch_reads: int = 1 << 20, with_profile: bool = False, paired: bool = True) -> dict:
        """What mcx_ctx_create_fit makes of this run on this device — everything the run takes allocated at once (context, tier 0's pair records, with_profile:
        planes and bookkeeping buffers), degraded until 4 GB of HBM stay free: pair records trimmed (the INDEX is changed: mcx_index_trim), batch halved —
        then given back.  Returns the mcx_fit record as a dict; the caller sizes its Mapper with ["max_batch_reads"]."""
        o = Opts()
        lib().mcx_opts_default(C.byref(o))
        o.alg = 0 if alg == "nw" else 1
        o.max_read_len, o.max_batch_reads = max_read_len, max_batch_reads
        h, planes, fit = C.c_void_p(), C.c_void_p(), Fit()
        _check(lib().mcx_ctx_create_fit(index._h, C.byref(o), int(with_profile), int(paired), 0, 5, C.byref(h), C.byref(planes) if with_profile else None, C.byref(fit)), "mcx_ctx_create_fit")
        if planes.value:
            lib().mcx_planes_free(planes)
        lib().mcx_ctx_free(h)
        return {k: int(getattr(fit, k)) for k, _ in Fit._fields_ if k != "pad"}

    def reset(self):
        lib().mcx_avg_init(self.avg)
        self.stats = Stats()

    # ---- whole path ---------------------------------------------------------------------
    def map_files(self, fq1: str, fq2: Optional[str], sam: Optional[str], interleaved: bool = False, threads: int = 0,
                  shard: Optional[Tuple[int, int]] = None, exchange: Optional[Exchange] = None, append_sam: bool = False,
                  device_sam: bool = False, device_inflate: bool = False, device_parse: bool = False, device_gz: bool = False, bgzf_sam: bool = False, bam: bool = False, sort: bool = False,
                  index: bool = False, markdup: bool = False, md: bool = False, read_group: Optional[str] = None, mate_tags: bool = False) -> dict:
        """Files in, SAM out (mcx_map_files_ex).  ``interleaved`` = -p, ``threads`` = -t; ``shard`` =
        (rank, count) with ``exchange``: map every count-th batch of the input stream while the shards
        keep one insert-size trajectory and one duplicate-cap order, and write the batches' lines at their
        final place in ``sam`` (the same path on every shard; shard 0 creates it).  The insert-size state
        (self.avg) carries over from call to call like the reference's globals (a new library starts a
        new 200-read chunk); ``append_sam``: a further library of the same run; ``device_sam`` = -gpu_sam: the
        SAM text is made on the device (the same bytes); ``device_inflate`` = -gpu_inflate: read files that are BGZF are inflated on the
        device (the same reads; other input is read as before); ``device_parse`` = -gpu_parse: plain FASTQ files, and plain FASTA files (one, or two as pairs; not sharded, not
        interleaved), are parsed and packed to 2-bit rows on the device (the same reads, the same end of the input; other input is read as before).
        ``device_inflate`` and ``device_parse`` together, on BGZF FASTQ or FASTA files (one, or two as pairs; not sharded, not interleaved, and with ``device_sam`` when a SAM file is written): the resident route — inflate,
        parse, pack, map and SAM text all in HBM.  ``device_gz`` = -gpu_gz: the same route for read files that are ORDINARY gzip streams (``device_gz`` and ``device_parse``; a pair may mix the two
        kinds when both switches are set); without ``device_parse``, and on files the block-start search cannot cut, the call runs as without it.  ``bgzf_sam`` = -bgzf: the SAM file is written as BGZF, its blocks deflated on the device (implies ``device_sam``; gzip -d of the
        file is the SAM file; not sharded: ERR_UNSUPPORTED).  ``bam`` = -bam: ``sam`` is written as BAM — the records made on the device, framed by the same BGZF path (implies both;
        unsorted, no index; not sharded).  ``sort`` = -sort, only with ``bam``: the file is coordinate-sorted (samtools sort's order, ties in input order) — every part's records sorted
        on the device into a run of a temporary file beside ``sam`` (removed again), the runs merged chunk by chunk on the device behind the last batch; ERR_UNSUPPORTED without ``bam``,
        with ``append_sam`` or sharded; ``sort_stats()`` says what the merge did.  ``index`` = -index, only with ``sort``: ``sam`` + ".bai" is written as well (what samtools index makes of the file), built on the
        device from the merge's chunks and written once the BAM file is complete; ERR_UNSUPPORTED without ``sort``, for ``sam`` "-" and for a contig longer than 2^29; ``index_stats()``
        says what was written.  ``markdup`` = -markdup, only with ``sort``: flag bit 0x400 on every record that is a duplicate (the rule: mcx.h at mcx_bam_dup_units_dev) — units made per
        part, resolved once on the device behind the last batch, the bits set in the merge; ERR_UNSUPPORTED without ``sort`` and on a mapper with ``multi``; ``markdup_stats()`` says what was found.
        ``md`` = -md: an MD:Z tag behind XS on every mapped line, its strings made on the device behind each part's mapping (mcx_md_dev) — with every output above and
        with the host formatter; ERR_UNSUPPORTED in a sharded run.
        ``read_group`` = -rg: an @RG line in bwa mem -R's form (``\\t`` or real TABs between the fields, exactly one ID; checked by rg_parse: ERR_ARG) that ends the header,
        and RG:Z:<ID> on every line; ``mate_tags`` = -mc: MC:Z and MQ:i on the lines of pairs whose mate is mapped and whose FLAG has 0x8 clear (the rule: mcx.h at
        mcx_sam_tags) — both with every output above and with the host formatter; ERR_UNSUPPORTED in a sharded run, ``mate_tags`` also on a mapper with ``multi``.
        BAM input: ``fq1`` a BGZF file whose text begins ``BAM\\1`` (any name), ``fq2`` None — the resident route by itself (the three device switches are implied for
        the call), pairs or single reads by the first taken record's flag 0x1 (``interleaved`` is ignored); ERR_UNSUPPORTED with a second file or in a sharded run,
        ERR_ARG when the mates are not neighbours; ``last_route()`` shows ROUTE_BAM_IN.
        ``last_route()`` says which stages ran on the device."""
        st = Stats()
        fo = FileOpts()
        lib().mcx_file_opts_default(C.byref(fo))
        fo.interleaved_pairs, fo.host_threads = int(interleaved), threads
        fo.append_sam = int(append_sam)
        fo.device_sam = (SAM_DEVICE if device_sam or bgzf_sam or bam else 0) | (SAM_BGZF if bgzf_sam or bam else 0) | (SAM_BAM if bam else 0) | (SAM_SORT if sort else 0) | (SAM_INDEX if index else 0) | (SAM_MARKDUP if markdup else 0) | (SAM_MD if md else 0) | (SAM_MC if mate_tags else 0)
        fo.device_inflate = (INFLATE_BGZF if device_inflate else 0) | (INFLATE_GZ if device_gz else 0)
        fo.device_parse = int(device_parse)
        if self.avg[3] % 200:
            self.avg[3] += 200 - self.avg[3] % 200
        fo.avg_state = C.cast(self.avg, C.POINTER(C.c_int64))
        if shard and shard[1] > 1:
            if exchange is None:
                raise ValueError("a sharded run needs an exchange (api.dist_exchange())")
            fo.shard_rank, fo.shard_count = int(shard[0]), int(shard[1])
            fo.exchange = C.pointer(exchange)
        rg = rg_parse(read_group)[0] if read_group is not None else None
        _check(lib().mcx_map_files_rg(self._h, fq1.encode(), (fq2 or "").encode() or None, C.byref(fo), rg, (sam or "").encode() or None,
                                      C.byref(st)), "mcx_map_files_ex")
        return st.as_dict()

    def last_route(self) -> Tuple[int, int]:
        """mcx_files_route: per read file of the last map_files call, the stages that ran on the device as a sum of ROUTE_INFLATE, ROUTE_PARSE, ROUTE_ROWS
        (the batches entered their slots from HBM), ROUTE_SAM, ROUTE_BGZF (the SAM text left the device as BGZF blocks), ROUTE_BAM (... of BAM records) and ROUTE_GZ (the file's ordinary gzip stream was inflated on the device); the second entry is 0 for one file."""
        r = (C.c_uint32 * 2)()
        _check(lib().mcx_files_route(self._h, r), "mcx_files_route")
        return int(r[0]), int(r[1])

    def submit_dev(self, d_codes_ptr: int, row_words: int, d_len_ptr: int, n_reads: int, d_odd_ptr: int, n_odd: int) -> None:
        """mcx_stream_submit_dev: mcx_stream_submit_packed's arguments as device pointers on the mapper's device (e.g. what FastqParser.parse_dev wrote to
        rows / len / odd); the buffers must hold their contents until the batch has been handed out (mcx_stream_next / mcx_stream_map*)."""
        _check(lib().mcx_stream_submit_dev(self._h, d_codes_ptr, row_words, d_len_ptr, n_reads, d_odd_ptr or None, n_odd), "mcx_stream_submit_dev")

    def map_batch(self, bases: np.ndarray, off: np.ndarray, paired: bool):
        """Host buffers: bases uint8 ASCII (concatenated), off uint32 [n+1].  Returns (aln, cigars): the records and, per
        read, its CIGAR words (aln[r].n_cigar of them, taken out of the batch's pool at aln[r].cigar_off)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint32)
        n = off.size - 1
        aln = np.zeros(n, dtype=ALN_DTYPE)
        pool = np.zeros(cigar_pool_words(n), dtype=np.uint32)
        _check(lib().mcx_map_batch(self._h, bases.ctypes.data, off.ctypes.data, n, int(paired), self.avg,
                                   aln.ctypes.data, pool.ctypes.data, C.byref(self.stats)), "mcx_map_batch")
        cigars = [pool[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])] for a in aln]
        if not self.multi:
            return aln, cigars
        return aln, cigars, self.multi_lines(n)

    def _md_into(self, si: "SamIn", keep: list) -> Tuple[np.ndarray, np.ndarray]:
        """mcx_md over the host arrays of ``si``: (the strings back to back, their n_reads + n_extras + 1 offsets), which si.md / si.md_off then point at"""
        n_x = int(np.ctypeslib.as_array(C.cast(si.x_index, C.POINTER(C.c_uint32)), shape=(si.n_reads + 1,))[-1]) if si.x_index and si.n_reads else 0
        md_off = np.zeros(si.n_reads + n_x + 1, dtype=np.uint32)
        nb = C.c_uint64()
        rc = lib().mcx_md(self._h, C.byref(si), None, 0, md_off.ctypes.data, C.byref(nb))
        if rc not in (0, ERR_CAPACITY):
            _check(rc, "mcx_md")
        md = np.zeros(max(1, nb.value), dtype=np.uint8)
        _check(lib().mcx_md(self._h, C.byref(si), md.ctypes.data, nb.value, md_off.ctypes.data, C.byref(nb)), "mcx_md")
        si.md, si.md_off = md.ctypes.data, md_off.ctypes.data
        keep += [md, md_off]
        return md[:nb.value], md_off

    def md_strings(self, bases: np.ndarray, off: np.ndarray, paired: bool, aln: np.ndarray, pool: np.ndarray, extras=None) -> List[Optional[bytes]]:
        """The MD:Z strings of a mapped batch, made on the device (mcx_md) from what sam_text takes (no names, no qualities): one entry per read's own
        record, then one per extra of ``extras`` in its order; None where the line gets no tag (unmapped, no CIGAR)."""
        n = np.asarray(off).size - 1
        si, keep = _sam_in(bases, off, [b""] * n, None, paired, aln, pool, extras)
        md, md_off = self._md_into(si, keep)
        buf = md.tobytes()
        return [buf[int(a):int(b)] if b > a else None for a, b in zip(md_off[:-1], md_off[1:])]

    def md_last_ms(self) -> Tuple[float, float, float]:
        """the last mcx_md[_dev]'s device times in ms: length kernel, scan, write kernel"""
        ms = (C.c_float * 3)()
        _check(lib().mcx_md_last_ms(self._h, ms), "mcx_md_last_ms")
        return ms[0], ms[1], ms[2]

    def sam_text(self, bases: np.ndarray, off: np.ndarray, names: List[bytes], quals: Optional[List[bytes]], paired: bool, aln: np.ndarray,
                 pool: np.ndarray, extras=None, md: bool = False, read_group: Optional[str] = None, mate_tags: bool = False) -> bytes:
        """The SAM lines of a mapped batch, made on the device (mcx_sam_format).  ``bases`` / ``off`` as given to map_batch, ``names`` the
        QNAMEs, ``quals`` per read the bytes of its quality line that count (at most the read's length; shorter ones are NUL-padded here;
        None: QUAL is '*'), ``aln`` the records and ``pool`` CIGAR words such that read r's are pool[aln[r].cigar_off:][:n_cigar] — map_batch's
        list of per-read arrays is accepted too —, ``extras`` what multi_lines returns.  ``md``: an MD:Z tag behind XS on every mapped line (mcx_md).
        ``read_group`` (an @RG line as map_files takes it): RG:Z:<ID> on every line; ``mate_tags``: MC:Z and MQ:i by the rule at mcx_sam_tags (not with ``extras``)."""
        si, keep = _sam_in(bases, off, names, quals, paired, aln, pool, extras)
        if md and si.n_reads:
            self._md_into(si, keep)
        tg = _sam_tags(read_group, mate_tags, keep)
        nb = C.c_uint64()
        rc = lib().mcx_sam_format_tags(self._h, C.byref(si), tg, None, 0, None, C.byref(nb))
        if rc not in (0, ERR_CAPACITY):
            _check(rc, "mcx_sam_format")
        text = np.zeros(max(1, nb.value), dtype=np.uint8)
        _check(lib().mcx_sam_format_tags(self._h, C.byref(si), tg, text.ctypes.data, nb.value, None, C.byref(nb)), "mcx_sam_format")
        return text[:nb.value].tobytes()

    def bam_records(self, bases: np.ndarray, off: np.ndarray, names: List[bytes], quals: Optional[List[bytes]], paired: bool, aln: np.ndarray,
                    pool: np.ndarray, extras=None, md: bool = False, read_group: Optional[str] = None, mate_tags: bool = False) -> Tuple[bytes, int]:
        """The uncompressed BAM records of a mapped batch, made on the device (mcx_bam_format), from what sam_text takes: (the records back to
        back — the record of every line sam_text would give, in its order —, the lines that made none: a name of 252 bytes or more, a QUAL that
        is not '*' and not as long as the read).  ``md``: an MD:Z tag behind XS in every mapped record (mcx_md);
        ``read_group`` and ``mate_tags`` as sam_text takes them: RG:Z, and MC:Z / MQ:i, behind it."""
        si, keep = _sam_in(bases, off, names, quals, paired, aln, pool, extras)
        if md and si.n_reads:
            self._md_into(si, keep)
        tg = _sam_tags(read_group, mate_tags, keep)
        nb, nd = C.c_uint64(), C.c_uint64()
        rc = lib().mcx_bam_format_tags(self._h, C.byref(si), tg, None, 0, None, C.byref(nb), C.byref(nd))
        if rc not in (0, ERR_CAPACITY):
            _check(rc, "mcx_bam_format")
        out = np.zeros(max(1, nb.value), dtype=np.uint8)
        _check(lib().mcx_bam_format_tags(self._h, C.byref(si), tg, out.ctypes.data, nb.value, None, C.byref(nb), C.byref(nd)), "mcx_bam_format")
        return out[:nb.value].tobytes(), int(nd.value)

    def sort_stats(self) -> dict:
        """mcx_files_sort_stats: what the last map_files(sort=True) did — runs, chunks, slices, slices that start inside a BGZF block, bytes read back from the
        temporary file, and how many of those twice (the blocks at slice borders)"""
        v = (C.c_uint64 * 6)()
        _check(lib().mcx_files_sort_stats(self._h, v), "mcx_files_sort_stats")
        return dict(zip(("runs", "chunks", "slices", "slices_inside_a_block", "bytes_read", "bytes_read_twice"), (int(x) for x in v)))

    def index_stats(self) -> dict:
        """mcx_files_index_stats: what the last map_files(index=True) wrote — stretches, bins, linear-index entries, the .bai file's bytes (all 0 after a run that failed)"""
        v = (C.c_uint64 * 4)()
        _check(lib().mcx_files_index_stats(self._h, v), "mcx_files_index_stats")
        return dict(zip(("stretches", "bins", "intervals", "bytes"), (int(x) for x in v)))

    def markdup_stats(self) -> dict:
        """mcx_files_markdup_stats: what the last map_files(markdup=True) found — pair units, duplicate pair units, fragment units, duplicate fragment units, groups
        (keys two or more pairs share, plus ends on which a fragment is a duplicate), seconds (all 0 after a run that failed)"""
        v = (C.c_uint64 * 6)()
        _check(lib().mcx_files_markdup_stats(self._h, v), "mcx_files_markdup_stats")
        d = dict(zip(("pairs", "duplicate_pairs", "fragments", "duplicate_fragments", "groups"), (int(x) for x in v)))
        d["seconds"] = int(v[5]) / 1e6
        return d

    def bam_dup_units(self, recs, grp_off, paired: bool):
        """mcx_bam_dup_units_dev over torch tensors on the mapper's device: ``recs`` uint8 — whole BAM records in read order —, ``grp_off`` 64-bit [n_groups + 1], the
        reads' offsets (mcx_bam_format_dev's rec_off).  Returns a uint8 tensor of 24 bytes a unit (view it as DUP_UNIT_DTYPE on the host): one unit per pair of
        groups when ``paired``, else per group."""
        import torch
        assert recs.dtype == torch.uint8 and recs.is_contiguous() and grp_off.element_size() == 8 and grp_off.is_contiguous()
        n_groups = max(0, grp_off.numel() - 1)
        units = torch.zeros(24 * max(1, n_groups), dtype=torch.uint8, device=recs.device)
        torch.cuda.synchronize()
        n = C.c_uint64()
        _check(lib().mcx_bam_dup_units_dev(self._h, recs.data_ptr() if recs.numel() else None, recs.numel(), grp_off.data_ptr(), n_groups, int(paired), units.data_ptr(), C.byref(n)),
               "mcx_bam_dup_units_dev")
        return units[:24 * n.value]

    def dup_resolve(self, units):
        """mcx_dup_resolve_dev: ``units`` as bam_dup_units returns them (or a host array of DUP_UNIT_DTYPE brought to the device as bytes); returns a uint8 tensor, one
        byte a unit: 1 for a duplicate"""
        import torch
        assert units.dtype == torch.uint8 and units.is_contiguous() and units.numel() % 24 == 0
        n = units.numel() // 24
        dup = torch.zeros(max(1, n), dtype=torch.uint8, device=units.device)
        torch.cuda.synchronize()
        _check(lib().mcx_dup_resolve_dev(self._h, units.data_ptr() if n else None, n, dup.data_ptr()), "mcx_dup_resolve_dev")
        return dup[:n]

    def bam_dup_mark(self, recs, rec_off, rec_dup) -> None:
        """mcx_bam_dup_mark_dev: flag bit 0x400 on record i of ``recs`` (uint8, in place; ``rec_off`` 64-bit [n + 1]) where ``rec_dup`` (uint8 [n]) is not 0"""
        import torch
        assert recs.dtype == torch.uint8 and recs.is_contiguous() and rec_off.element_size() == 8 and rec_off.is_contiguous() and rec_dup.dtype == torch.uint8 and rec_dup.is_contiguous()
        n = max(0, rec_off.numel() - 1)
        assert rec_dup.numel() >= n
        torch.cuda.synchronize()
        _check(lib().mcx_bam_dup_mark_dev(self._h, recs.data_ptr() if recs.numel() else None, recs.numel(), rec_off.data_ptr(), n, rec_dup.data_ptr()), "mcx_bam_dup_mark_dev")

    def markdup_last_ms(self) -> Tuple[float, float, float]:
        """the device times in ms of the last mcx_bam_dup_units_dev, mcx_dup_resolve_dev and mcx_bam_dup_mark_dev"""
        ms = (C.c_float * 3)()
        _check(lib().mcx_markdup_last_ms(self._h, ms), "mcx_markdup_last_ms")
        return tuple(float(x) for x in ms)

    def bam_index(self, recs, rec_off, block: int, block_coff, lin, lin_base, runs=None):
        """mcx_bam_index_dev over torch tensors on the mapper's device: ``recs`` uint8 — coordinate-sorted BAM records back to back —, ``rec_off`` 64-bit [n + 1], their
        offsets from 0 to recs.numel(); ``block`` the bytes of text a BGZF block took and ``block_coff`` 64-bit [n_blocks + 1] where each block lies in the file;
        ``lin`` 64-bit, the windows' table (all-ones before the first call; updated in place), and ``lin_base`` 64-bit [n_ref + 1], where each contig's windows begin
        in it.  Returns the stretches as a numpy array of BAI_RUN_DTYPE; ``runs``: a uint8 tensor of 24 bytes a stretch to take them (ERR_CAPACITY when it is short;
        default: as many as there are records)."""
        import torch
        for t in (rec_off, block_coff, lin, lin_base):
            assert t.element_size() == 8 and t.is_contiguous(), "offsets and tables: 64-bit tensors"
        assert recs.dtype == torch.uint8 and recs.is_contiguous()
        n = max(0, rec_off.numel() - 1)
        if runs is None:
            runs = torch.zeros(24 * max(n, 1), dtype=torch.uint8, device=recs.device)
        assert runs.dtype == torch.uint8 and runs.is_contiguous()
        torch.cuda.synchronize()
        n_runs = C.c_uint64()
        _check(lib().mcx_bam_index_dev(self._h, recs.data_ptr() if recs.numel() else None, recs.numel(), rec_off.data_ptr(), n, block, block_coff.data_ptr(), max(0, block_coff.numel() - 1),
                                       lin.data_ptr(), lin_base.data_ptr(), max(0, lin_base.numel() - 1), runs.data_ptr(), runs.numel() // 24, C.byref(n_runs)), "mcx_bam_index_dev")
        return runs[:24 * n_runs.value].cpu().numpy().view(BAI_RUN_DTYPE).copy()

    def bam_index_last_ms(self) -> Tuple[float, float, float]:
        """the last mcx_bam_index_dev's device times in ms: records, stretches, windows"""
        ms = (C.c_float * 3)()
        _check(lib().mcx_bam_index_last_ms(self._h, ms), "mcx_bam_index_last_ms")
        return tuple(float(x) for x in ms)

    def bam_sort(self, recs, grp_off, keys=None, lens=None, out=None):
        """mcx_bam_sort_dev over torch tensors on the mapper's device: ``recs`` uint8 — whole BAM records back to back —, ``grp_off`` int64 / uint64 [n_groups + 1], the
        groups' offsets (mcx_bam_format_dev's rec_off).  Returns (the records in coordinate order — ``out`` or a new uint8 tensor of recs' size —, the number of
        records); ``keys`` (int64, viewed as uint64) and ``lens`` (int32) receive each output record's key and length when given (room for recs.numel() // 36)."""
        import torch
        assert recs.dtype == torch.uint8 and recs.is_contiguous() and grp_off.element_size() == 8 and grp_off.is_contiguous()
        if out is None:
            out = torch.empty_like(recs)
        assert out.dtype == torch.uint8 and out.is_contiguous()
        assert keys is None or (keys.element_size() == 8 and keys.is_contiguous()), "keys: a 64-bit tensor"
        assert lens is None or (lens.element_size() == 4 and lens.is_contiguous()), "lens: a 32-bit tensor"
        torch.cuda.synchronize()
        n = C.c_uint64()
        _check(lib().mcx_bam_sort_dev(self._h, recs.data_ptr() if recs.numel() else None, recs.numel(), grp_off.data_ptr(), max(0, grp_off.numel() - 1),
                                      out.data_ptr() if out.numel() else None, out.numel(), keys.data_ptr() if keys is not None else None,
                                      lens.data_ptr() if lens is not None else None, C.byref(n)), "mcx_bam_sort_dev")
        return out, int(n.value)

    def bam_sort_last_ms(self) -> Tuple[float, float, float, float]:
        """the last mcx_bam_sort_dev's device times in ms: index, sort, place, gather"""
        ms = (C.c_float * 4)()
        _check(lib().mcx_bam_sort_last_ms(self._h, ms), "mcx_bam_sort_last_ms")
        return tuple(float(x) for x in ms)

    def pass_last_shape(self) -> dict:
        """mcx_pass_last_shape: the last tier-0 pass — the pairs the order listed per weight class (heaviest first; all zero without the order), the pairs of
        the heavy and of the light clustering launch, whether the heavy ones went aside (a side stream beside the straight-line path), the early list's length"""
        v = (C.c_uint32 * 10)()
        _check(lib().mcx_pass_last_shape(self._h, v), "mcx_pass_last_shape")
        return {"classes": [int(x) for x in v[:6]], "heavy": int(v[6]), "light": int(v[7]), "aside": int(v[8]), "early": int(v[9])}

    def bam_last_ms(self) -> Tuple[float, float, float]:
        """the last mcx_bam_format[_dev]'s device times in ms: length kernel, scan, write kernel"""
        ms = (C.c_float * 3)()
        _check(lib().mcx_bam_last_ms(self._h, ms), "mcx_bam_last_ms")
        return float(ms[0]), float(ms[1]), float(ms[2])

    def multi_lines(self, n_reads: int):
        """(multi) the last batch's extra lines: (index uint32 [n_reads + 1], records ALN_DTYPE, their CIGAR words per record) — read r's
        lines after its first are records[index[r]:index[r + 1]], in the order the reference prints them (mcx_multi_lines / mcx_multi_copy)."""
        if n_reads == 0:
            return np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=ALN_DTYPE), []
        nl, nw = C.c_uint32(), C.c_uint32()
        _check(lib().mcx_multi_lines(self._h, None, None, None, C.byref(nl), C.byref(nw)), "mcx_multi_lines")
        index = np.zeros(n_reads + 1, dtype=np.uint32)
        recs = np.zeros(nl.value, dtype=ALN_DTYPE)
        words = np.zeros(max(1, nw.value), dtype=np.uint32)
        _check(lib().mcx_multi_copy(self._h, index.ctypes.data, recs.ctypes.data, words.ctypes.data), "mcx_multi_copy")
        return index, recs, [words[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])] for a in recs]

    @staticmethod
    def stream_outputs(n_reads: int, slots: int = 3, record_bytes: int = 64):
        """Pinned host buffers for map_stream's results: [(records uint8[n_reads * record_bytes], CIGAR pool int32[cigar_pool_words(n_reads)])];
        record_bytes = 32: the records as mcx_aln32 (map_stream_packed(..., out32=True): half the bytes on the way out)."""
        import torch
        return [(torch.empty(n_reads * record_bytes, dtype=torch.uint8).pin_memory(), torch.empty(cigar_pool_words(n_reads), dtype=torch.int32).pin_memory())
                for _ in range(slots)]

    def map_stream(self, host_bases_ptrs, host_off_ptr: int, n_reads: int, paired: bool, outputs=None):
        """A sequence of equally shaped batches from pinned host memory, results to pinned host memory, the copies of one
        batch overlapped with the kernels of its neighbours (mcx_stream_*).  ``outputs``: stream_outputs() (batch i lands in
        slot i % len).  Returns (bytes copied in, bytes copied out)."""
        L = lib()
        k = len(host_bases_ptrs)
        outs = outputs or self.stream_outputs(n_reads, min(k, 3))
        h2d = C.c_uint64()
        d2h = C.c_uint64()
        for i in range(k + 2):  # submit(i); map(i - 1); collect(i - 2)
            if i < k:
                _check(L.mcx_stream_submit(self._h, host_bases_ptrs[i], host_off_ptr, n_reads), "mcx_stream_submit")
            if 1 <= i <= k:
                a, g = outs[(i - 1) % len(outs)]
                _check(L.mcx_stream_map(self._h, int(paired), self.avg, a.data_ptr(), g.data_ptr(), C.byref(self.stats)), "mcx_stream_map")
            if i >= 2:
                _check(L.mcx_stream_collect(self._h, C.byref(h2d), C.byref(d2h)), "mcx_stream_collect")
                if self.multi:
                    self.stream_multi.append(self.stream_multi_collected())
        return h2d.value, d2h.value

    def map_stream_packed(self, packed, n_reads: int, paired: bool, outputs=None, out32: bool = False):
        """map_stream with the reads as a host parser packs them (pack_reads): ``packed`` = [(codes ptr, row_words, len ptr, odd ptr, n_odd)]
        per batch, all in pinned host memory."""
        L = lib()
        k = len(packed)
        outs = outputs or self.stream_outputs(n_reads, min(k, 3), 32 if out32 else 64)
        h2d = C.c_uint64()
        d2h = C.c_uint64()
        stream_map = L.mcx_stream_map32 if out32 else L.mcx_stream_map
        for i in range(k + 2):
            if i < k:
                codes, row_words, lens, odd, n_odd = packed[i]
                _check(L.mcx_stream_submit_packed(self._h, codes, row_words, lens, n_reads, odd, n_odd), "mcx_stream_submit_packed")
            if 1 <= i <= k:
                a, g = outs[(i - 1) % len(outs)]
                _check(stream_map(self._h, int(paired), self.avg, a.data_ptr(), g.data_ptr(), C.byref(self.stats)), "mcx_stream_map")
            if i >= 2:
                _check(L.mcx_stream_collect(self._h, C.byref(h2d), C.byref(d2h)), "mcx_stream_collect")
                if self.multi:
                    self.stream_multi.append(self.stream_multi_collected())
        return h2d.value, d2h.value

    def stream_multi_collected(self):
        """(multi) the extras of the batch the last mcx_stream_collect handed over, copied out of the slot's page-locked buffers:
        (index uint32 [n_reads + 1], records ALN_DTYPE, their CIGAR words per record) as multi_lines gives them."""
        idx, recs, cig = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nr, nl, nw = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().mcx_stream_multi(self._h, C.byref(idx), C.byref(recs), C.byref(cig), C.byref(nr), C.byref(nl), C.byref(nw)), "mcx_stream_multi")
        if nr.value == 0:
            return np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=ALN_DTYPE), []
        index = np.ctypeslib.as_array(C.cast(idx, C.POINTER(C.c_uint32)), (nr.value + 1,)).copy()
        a32 = np.frombuffer(C.string_at(recs, nl.value * ALN32_DTYPE.itemsize), dtype=ALN32_DTYPE) if nl.value else np.zeros(0, dtype=ALN32_DTYPE)
        words = np.ctypeslib.as_array(C.cast(cig, C.POINTER(C.c_uint32)), (nw.value,)).copy() if nw.value else np.zeros(1, dtype=np.uint32)
        out = aln32_unpack(a32)
        return index, out, [words[int(a["cigar_off"]):int(a["cigar_off"]) + int(a["n_cigar"])] for a in out]

    def map_batch_dev(self, d_bases_ptr: int, d_off_ptr: int, n_reads: int, paired: bool, d_aln_ptr: int, d_cigar_ptr: int):
        """Device pointers (e.g. torch.Tensor.data_ptr()); results stay in HBM."""
        _check(lib().mcx_map_batch_dev(self._h, d_bases_ptr, d_off_ptr, n_reads, int(paired), self.avg, d_aln_ptr,
                                       d_cigar_ptr, C.byref(self.stats)), "mcx_map_batch_dev")

    # ---- a batch in steps (runs whose batches are mapped by several GPUs) ---------------------
    def batch_begin(self, d_bases_ptr: int, d_off_ptr: int, n_reads: int, paired: bool, est0: int, read_base: int, d_aln_ptr: int, d_cigar_ptr: int):
        _check(lib().mcx_batch_begin(self._h, d_bases_ptr, d_off_ptr, n_reads, int(paired), est0, read_base, d_aln_ptr, d_cigar_ptr,
                                     C.byref(self.stats)), "mcx_batch_begin")

    def batch_sums(self):
        """(pairs, dist, len) per chunk of 100 pairs: uint32 numpy views, valid until the next call on the context."""
        n = C.c_uint32()
        p = [C.POINTER(C.c_uint32)() for _ in range(3)]
        _check(lib().mcx_batch_sums(self._h, C.byref(n), C.byref(p[0]), C.byref(p[1]), C.byref(p[2])), "mcx_batch_sums")
        return tuple(np.ctypeslib.as_array(q, shape=(n.value,)) if n.value else np.zeros(0, np.uint32) for q in p)

    def batch_replay(self, est_chunk: np.ndarray) -> int:
        est_chunk = np.ascontiguousarray(est_chunk, dtype=np.int32)
        n = C.c_uint32()
        _check(lib().mcx_batch_replay(self._h, est_chunk.ctypes.data, C.byref(n), C.byref(self.stats)), "mcx_batch_replay")
        return n.value

    def batch_totals(self) -> Tuple[int, int]:
        """(proper pairs, their summed distance) of the batch as it stands: what the shards of a round tell each other."""
        t = (C.c_int64 * 2)()
        _check(lib().mcx_batch_totals(self._h, t), "mcx_batch_totals")
        return int(t[0]), int(t[1])

    def batch_check(self, state_before, first_of_round: bool) -> int:
        """The chunks of the batch against the trajectory that starts from ``state_before`` = (avgDist at the round's start, pairs and
        distance before this batch's first chunk); the pairs whose estimate moved are re-run.  Returns how many."""
        st = (C.c_int64 * 3)(*[int(v) for v in state_before])
        n = C.c_uint32()
        _check(lib().mcx_batch_check(self._h, st, 1 if first_of_round else 0, C.byref(n), C.byref(self.stats)), "mcx_batch_check")
        return n.value

    def batch_end(self):
        _check(lib().mcx_batch_end(self._h, C.byref(self.stats)), "mcx_batch_end")

    # ---- -vcf bookkeeping ---------------------------------------------------------------
    def profile_attach(self, d_planes_ptr: int, max_dup: int = 5, max_clip: int = 5) -> None:
        """d_planes: zeroed device memory of planes_words(GenomeSize) 32-bit words (planes_alloc), caller-owned so
        that it can be reduced across GPUs; every later map_batch* call accumulates into it."""
        _check(lib().mcx_profile_attach(self._h, d_planes_ptr, max_dup, max_clip), "mcx_profile_attach")

    def profile_settle(self) -> None:
        """The planes kept as differences while the run is mapped become counts: once, after the last
        batch and before the planes are read or reduced over the ranks (implied by profile_finalize)."""
        _check(lib().mcx_profile_settle(self._h), "mcx_profile_settle")

    def profile_finalize(self, d_planes_ptr: int) -> None:
        _check(lib().mcx_profile_finalize(self._h, d_planes_ptr), "mcx_profile_finalize")

    def profile_sparse_raw(self, shard: bool = False, copy: bool = True) -> np.ndarray:
        """The same records as they are (uint8 [n, 64] copies of mcx_sparse_rec), for all-gathers
        and for Index.call_variants without a Python loop.  ``shard``: the form for a run spread over
        several shards (discordant-pair events 'E' instead of the sites they resolve to).  ``copy=False``:
        a view of the library's own array — valid until the next profile_* call or close()."""
        recs = C.POINTER(SparseRec)()
        n = C.c_uint64()
        f = lib().mcx_profile_sparse_shard if shard else lib().mcx_profile_sparse
        _check(f(self._h, C.byref(recs), C.byref(n)), "mcx_profile_sparse")
        if n.value == 0:
            return np.zeros((0, 64), dtype=np.uint8)
        buf = (C.c_uint8 * (64 * n.value)).from_address(C.addressof(recs.contents))
        view = np.frombuffer(buf, dtype=np.uint8).reshape(n.value, 64)
        return view.copy() if copy else view

    def profile_sparse(self):
        """[(type, pos, seq or dist)]: 'I'/'D'/'B' events and 'V'/'T' discordant-site records."""
        recs = C.POINTER(SparseRec)()
        n = C.c_uint64()
        _check(lib().mcx_profile_sparse(self._h, C.byref(recs), C.byref(n)), "mcx_profile_sparse")
        out = []
        for i in range(n.value):
            r = recs[i]
            t = chr(r.type)
            if t in "VT":
                out.append((t, int(r.pos), int.from_bytes(C.string_at(C.addressof(r) + 10, 8), "little", signed=True)))
            elif t == "C":  # the string of the record before continues
                pt, pp, ps = out[-1]
                out[-1] = (pt, pp, ps + C.string_at(C.addressof(r) + 10, min(r.len, 54)).decode("latin-1"))
            else:
                out.append((t, int(r.pos), C.string_at(C.addressof(r) + 10, min(r.len, 54)).decode("latin-1")))
        return out

    # ---- per-call drop-ins --------------------------------------------------------------
    def bwt_search(self, seqs: List[bytes], starts: List[int]):
        """BWT_Search for many (code string, start) queries. Returns (len, freq, loc[n,50])."""
        n = len(seqs)
        off = np.zeros(n + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(s) for s in seqs])
        buf = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
        st = np.asarray(starts, dtype=np.int32)
        ln = np.zeros(n, dtype=np.int32)
        fr = np.zeros(n, dtype=np.int32)
        loc = np.zeros((n, 50), dtype=np.uint64)
        _check(lib().mcx_bwt_search_batch(self._h, buf.ctypes.data, off.ctypes.data, st.ctypes.data, n, ln.ctypes.data,
                                          fr.ctypes.data, loc.ctypes.data), "mcx_bwt_search_batch")
        return ln, fr, loc

    def seed_walk(self, seqs: List[bytes], fm_budget: int = 1 << 30, cap: int = 1024):
        """The greedy seeding walk of each read (ASCII bases) as the seeding kernel runs it (mcx_seed_walk_batch).  Returns
        (n_hits[n], hits[n, cap] with fields gPos, rPos, len): read i's first min(n_hits[i], cap) seeds in the walk's order."""
        n = len(seqs)
        off = np.zeros(n + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(s) for s in seqs])
        buf = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
        n_hits = np.zeros(n, dtype=np.int32)
        hits = np.zeros((n, cap), dtype=np.dtype([("gPos", np.int64), ("rPos", np.int32), ("len", np.int32)]))
        _check(lib().mcx_seed_walk_batch(self._h, buf.ctypes.data, off.ctypes.data, n, int(fm_budget), int(cap), n_hits.ctypes.data,
                                         hits.ctypes.data), "mcx_seed_walk_batch")
        return n_hits, hits

    def extend(self, alg: str, qs: List[bytes], ts: List[bytes]):
        """nw_alignment / ksw2_alignment for many (read fragment, genome fragment) pairs (ASCII).
        Returns (list of op strings of 'M','I','D', scores)."""
        n = len(qs)
        qo = np.zeros(n + 1, dtype=np.uint32)
        to = np.zeros(n + 1, dtype=np.uint32)
        qo[1:] = np.cumsum([len(s) for s in qs])
        to[1:] = np.cumsum([len(s) for s in ts])
        qb = np.frombuffer(b"".join(qs), dtype=np.uint8).copy()
        tb = np.frombuffer(b"".join(ts), dtype=np.uint8).copy()
        ops = np.zeros(int(qo[-1]) + int(to[-1]) + 16, dtype=np.uint8)
        ol = np.zeros(n, dtype=np.int32)
        sc = np.zeros(n, dtype=np.int32)
        _check(lib().mcx_extend_batch(self._h, 0 if alg == "nw" else 1, qb.ctypes.data, qo.ctypes.data, tb.ctypes.data,
                                      to.ctypes.data, n, ops.ctypes.data, ol.ctypes.data, sc.ctypes.data), "mcx_extend_batch")
        out = []
        for i in range(n):
            b = int(qo[i]) + int(to[i])
            out.append(ops[b:b + int(ol[i])].tobytes().decode())
        return out, sc

    def extend_lanes(self, alg: str, form: int, strip: int, qs: List[bytes], ts: List[bytes], blocks: int = 0, summaries: bool = False):
        """The same problems through the lane forms of the DP (mcx_extend_lanes), in the order given: form 1 = one problem per lane,
        2 = two per lane; strips of 8 or 16 target columns; blocks = wavefronts launched (0: one per group of 64 / 128 problems).
        Returns (op strings, their lengths as the kernel reports them, scores, DP_SUMMARY_DTYPE records or None)."""
        n = len(qs)
        qo = np.zeros(n + 1, dtype=np.uint32)
        to = np.zeros(n + 1, dtype=np.uint32)
        qo[1:] = np.cumsum([len(s) for s in qs])
        to[1:] = np.cumsum([len(s) for s in ts])
        qb = np.frombuffer(b"".join(qs) + b"\0", dtype=np.uint8).copy()
        tb = np.frombuffer(b"".join(ts) + b"\0", dtype=np.uint8).copy()
        ops = np.zeros(int(qo[-1]) + int(to[-1]) + 16, dtype=np.uint8)
        ol = np.zeros(n, dtype=np.int32)
        sc = np.zeros(n, dtype=np.int32)
        sm = np.zeros(n, dtype=DP_SUMMARY_DTYPE) if summaries else None
        _check(lib().mcx_extend_lanes(self._h, 0 if alg == "nw" else 1, form, strip, blocks, qb.ctypes.data, qo.ctypes.data, tb.ctypes.data,
                                      to.ctypes.data, n, ops.ctypes.data, ol.ctypes.data, sc.ctypes.data, sm.ctypes.data if summaries else None),
               "mcx_extend_lanes")
        out = []
        for i in range(n):
            b = int(qo[i]) + int(to[i])
            out.append(ops[b:b + int(ol[i])].tobytes().decode())
        return out, ol, sc, sm

    def close(self):
        if self._h:
            lib().mcx_ctx_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Inflater:
    """mcx_inflater: BGZF members (raw deflate streams of at most 64 KB of text each) inflated and CRC-checked on the device, a wavefront per
    member, on a stream of the object's own.  The capacities are those of one launch through host buffers (0: defaults, 8 MB of text)."""

    def __init__(self, device: int = 0, max_src_bytes: int = 0, max_dst_bytes: int = 0, max_members: int = 0):
        self._h = C.c_void_p()
        _check(lib().mcx_inflater_create(device, max_src_bytes, max_dst_bytes, max_members, C.byref(self._h)), "mcx_inflater_create")

    def close(self):
        if self._h:
            lib().mcx_inflater_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def inflate_dev(self, d_src, d_members, n: int, d_dst, d_status) -> int:
        """mcx_inflate_dev on torch tensors of the inflater's device: d_src uint8, d_members n records of MEMBER_DTYPE as bytes, d_dst uint8,
        d_status n 32-bit words (mcx_inflate_status).  Returns 0, ERR_IO when a member failed, ERR_ARG for members that break the contract."""
        rc = lib().mcx_inflate_dev(self._h, d_src.data_ptr(), d_src.numel(), d_members.data_ptr(), n, d_dst.data_ptr(), d_dst.numel(), d_status.data_ptr())
        if rc not in (0, ERR_IO, ERR_ARG):
            _check(rc, "mcx_inflate_dev")
        return rc

    def inflate(self, src, members: np.ndarray, dst: np.ndarray):
        """mcx_inflate on host buffers: src bytes, members of MEMBER_DTYPE, dst uint8 (written in place).  Returns (rc, status words)."""
        src = np.frombuffer(src, dtype=np.uint8) if not isinstance(src, np.ndarray) else src
        members = np.ascontiguousarray(members, dtype=MEMBER_DTYPE)
        status = np.zeros(members.size, dtype=np.uint32)
        rc = lib().mcx_inflate(self._h, src.ctypes.data, src.size, members.ctypes.data, members.size, dst.ctypes.data, dst.size, status.ctypes.data)
        if rc not in (0, ERR_IO, ERR_ARG):
            _check(rc, "mcx_inflate")
        return rc, status

    def last_ms(self) -> float:
        """the last inflate_dev's kernel, in ms by events on the inflater's stream"""
        ms = C.c_float()
        _check(lib().mcx_inflate_last_ms(self._h, C.byref(ms)), "mcx_inflate_last_ms")
        return float(ms.value)


class Gunzipper:
    """mcx_gunzipper: an ordinary gzip member's deflate stream inflated on the device a round at a time — block starts searched for in stretches of
    ``stretch_bytes`` compressed bytes (0: 64 KB), a wavefront per stretch inflating into 16-bit symbols, the 32 KB windows resolved along the chain, the
    text and its CRC-32 made in parallel (mcx.h).  ``max_stretches`` (0: 2048) a round; ``arena_symbols`` (0: 8 per compressed byte of a full round)."""

    def __init__(self, device: int = 0, stretch_bytes: int = 0, max_stretches: int = 0, arena_symbols: int = 0):
        self._h = C.c_void_p()
        _check(lib().mcx_gunzipper_create(device, stretch_bytes, max_stretches, arena_symbols, C.byref(self._h)), "mcx_gunzipper_create")

    def close(self):
        if self._h:
            lib().mcx_gunzipper_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        """a new member begins: no window"""
        lib().mcx_gunzipper_reset(self._h)

    def round_dev(self, d_src, at: int, src_bytes: int, start_bit: int, src_is_end: bool) -> GzRound:
        """mcx_gunzip_round_dev over d_src[at .. at + src_bytes), a uint8 torch tensor on the object's device that holds 8 bytes more behind them."""
        assert at + src_bytes + 8 <= d_src.numel()
        info = GzRound()
        _check(lib().mcx_gunzip_round_dev(self._h, d_src.data_ptr() + at, src_bytes, start_bit, int(src_is_end), C.byref(info)), "mcx_gunzip_round_dev")
        return info

    def text_dev(self, d_dst, info: GzRound) -> GzRound:
        """mcx_gunzip_text_dev: the last round's text into d_dst[0 .. info.text_bytes) (a uint8 torch tensor); info.crc32 and info.ms[3] are filled in."""
        _check(lib().mcx_gunzip_text_dev(self._h, d_dst.data_ptr(), d_dst.numel(), C.byref(info)), "mcx_gunzip_text_dev")
        return info


class FastqParser:
    """mcx_fastq_parser: FASTQ text parsed on the device (set_rule: the plain rule — getline's lines, the default — or the .gz readers', FASTQ_RULE_GZ) — record boundaries, names, bases, NUL-padded qualities, 2-bit rows and the list of
    bytes that are not ACGT — on a stream of the object's own.  max_text_bytes / max_records size the first scratch (0: defaults); it grows on demand.
    Both calls take the texts (one, or the two of a pair) and the outputs by keyword: recs (a list, one array of REC_DTYPE records per text), bases,
    off, qual, names, name_off, rows, len, odd — a group that is left out is not produced.  A capacity defaults to its array's size (bases_cap,
    names_cap in bytes, odd_cap in entries), row_words to the rows' second dimension and a text's length to its array's size (text_bytes: a list
    that says otherwise).  They return (rc, info): rc 0, ERR_ARG or ERR_CAPACITY;
    info a dict of mcx_fastq_info."""

    def __init__(self, device: int = 0, max_text_bytes: int = 0, max_records: int = 0):
        self._h = C.c_void_p()
        _check(lib().mcx_fastq_parser_create(device, max_text_bytes, max_records, C.byref(self._h)), "mcx_fastq_parser_create")

    def close(self):
        if self._h:
            lib().mcx_fastq_parser_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_rule(self, rule: int) -> None:
        """mcx_fastq_parser_set_rule: FASTQ_RULE_PLAIN or FASTQ_RULE_GZ for the calls that follow"""
        _check(lib().mcx_fastq_parser_set_rule(self._h, rule), "mcx_fastq_parser_set_rule")

    def set_format(self, fmt: int) -> None:
        """mcx_fastq_parser_set_format: READS_FASTQ (the default) or READS_FASTA for the calls that follow (FASTA: no qualities; under the plain rule multi-line records)"""
        _check(lib().mcx_fastq_parser_set_format(self._h, fmt), "mcx_fastq_parser_set_format")

    def set_reads(self, fmt: int) -> None:
        """mcx_fastq_parser_set_reads: set_format for all three formats — READS_FASTQ, READS_FASTA or READS_BAM (one text, the records behind the file's header; the
        calls take n_ref=...)"""
        _check(lib().mcx_fastq_parser_set_reads(self._h, fmt), "mcx_fastq_parser_set_reads")

    def set_mates(self, mates: bool) -> None:
        """mcx_fastq_parser_set_mates: under READS_BAM, taken records count in twos (0x1 | 0x40, then 0x1 | 0x80, equal names) for the calls that follow"""
        _check(lib().mcx_fastq_parser_set_mates(self._h, int(mates)), "mcx_fastq_parser_set_mates")

    def bam_last(self) -> dict:
        """mcx_bam_reads_last: the last READS_BAM call's counters"""
        st = (C.c_uint64 * 6)()
        _check(lib().mcx_bam_reads_last(self._h, st), "mcx_bam_reads_last")
        return dict(zip(("walked", "taken", "skipped", "first_flag", "chunks", "off_chain"), (int(x) for x in st)))

    def bam_last_ms(self) -> tuple:
        """mcx_bam_reads_last_ms: the last READS_BAM call's (search, walk, join, unpack) on the device, in ms"""
        ms = (C.c_float * 4)()
        _check(lib().mcx_bam_reads_last_ms(self._h, ms), "mcx_bam_reads_last_ms")
        return tuple(float(x) for x in ms)

    @staticmethod
    def _structs(ptr, size, texts, max_records, max_read_len, final, o):
        fi, fo = FastqIn(), FastqOut()
        text_bytes = o.get("text_bytes")
        for t, x in enumerate(texts):
            fi.text[t], fi.bytes[t] = ptr(x), size(x) if text_bytes is None else text_bytes[t]
        fi.max_records, fi.max_read_len, fi.final, fi.n_ref = max_records, max_read_len, int(final), o.get("n_ref", 0)
        for t, x in enumerate(o.get("recs") or []):
            fo.recs[t] = ptr(x) if x is not None else None
        for k in ("bases", "off", "qual", "names", "name_off", "rows", "len", "odd"):
            if o.get(k) is not None:
                setattr(fo, k, ptr(o[k]))
        fo.bases_cap = o.get("bases_cap", size(o["bases"]) if o.get("bases") is not None else 0)
        fo.names_cap = o.get("names_cap", size(o["names"]) if o.get("names") is not None else 0)
        fo.odd_cap = o.get("odd_cap", size(o["odd"]) if o.get("odd") is not None else 0)
        fo.row_words = o.get("row_words", o["rows"].shape[1] if o.get("rows") is not None and len(o["rows"].shape) == 2 else 0)
        return fi, fo

    def _call(self, f, name, fi, fo):
        info = FastqInfo()
        rc = f(self._h, C.byref(fi), C.byref(fo), C.byref(info))
        if rc not in (0, ERR_ARG, ERR_CAPACITY):
            _check(rc, name)
        return rc, info.as_dict()

    def parse_dev(self, texts, max_records: int, max_read_len: int, final: bool = True, **out):
        """mcx_fastq_parse_dev on torch tensors of the parser's device: texts uint8 (any alignment: a slice will do), recs uint8 tensors of 24 bytes a
        record, off / name_off / rows / len int32, odd int64.  The second text of a pair counts as long as it has an address: give an empty one as an empty
        slice of a larger tensor."""
        fi, fo = self._structs(lambda x: x.data_ptr() or None, lambda x: x.numel(), texts, max_records, max_read_len, final, out)
        return self._call(lib().mcx_fastq_parse_dev, "mcx_fastq_parse_dev", fi, fo)

    def parse(self, texts, max_records: int, max_read_len: int, final: bool = True, **out):
        """mcx_fastq_parse on host buffers: texts bytes or uint8 arrays, the outputs numpy arrays written in place."""
        keep = [np.frombuffer(x, dtype=np.uint8) if not isinstance(x, np.ndarray) else x for x in texts]
        keep = [x if x.size else np.zeros(1, dtype=np.uint8)[:0] for x in keep]
        fi, fo = self._structs(lambda x: x.ctypes.data, lambda x: x.size, keep, max_records, max_read_len, final, out)
        return self._call(lib().mcx_fastq_parse, "mcx_fastq_parse", fi, fo)

    def last_ms(self) -> float:
        """the last parse_dev on the device, in ms by events on the parser's stream"""
        ms = C.c_float()
        _check(lib().mcx_fastq_last_ms(self._h, C.byref(ms)), "mcx_fastq_last_ms")
        return float(ms.value)

    def grown(self) -> int:
        """how often one of the parser's buffers had to be replaced by a larger one"""
        n = C.c_uint32()
        _check(lib().mcx_fastq_grown(self._h, C.byref(n)), "mcx_fastq_grown")
        return int(n.value)


def bam_reads_header(data) -> tuple:
    """mcx_bam_reads_header over a BAM file's inflated bytes: (rc, records_at, n_ref) — rc 0, 1 (too few bytes) or -1 (no BAM)"""
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    at, n_ref = C.c_uint64(), C.c_int32()
    rc = lib().mcx_bam_reads_header(buf.ctypes.data, len(data), C.byref(at), C.byref(n_ref))
    return rc, int(at.value), int(n_ref.value)


class Deflater:
    """mcx_deflater: text compressed to BGZF blocks on the device, a wavefront per block of at most 65 280 bytes of text (set_block: fewer), on a stream of the
    object's own.  max_text_bytes: what one launch through host buffers takes (0: 8 MB).  The same text and block size give the same bytes on every run."""

    def __init__(self, device: int = 0, max_text_bytes: int = 0):
        self._h = C.c_void_p()
        self.block = BGZF_BLOCK
        _check(lib().mcx_deflater_create(device, max_text_bytes, C.byref(self._h)), "mcx_deflater_create")

    def close(self):
        if self._h:
            lib().mcx_deflater_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_block(self, text_bytes: int) -> int:
        """mcx_deflater_set_block: the bytes of text per block of the following calls (1 .. 65280).  Returns 0 or ERR_ARG."""
        rc = lib().mcx_deflater_set_block(self._h, text_bytes)
        if rc == 0:
            self.block = text_bytes
        elif rc != ERR_ARG:
            _check(rc, "mcx_deflater_set_block")
        return rc

    def bound(self, text_bytes: int) -> int:
        return int(lib().mcx_bgzf_bound(text_bytes, self.block))

    def deflate_dev(self, d_text, text_bytes: int, d_out, out_cap: Optional[int] = None):
        """mcx_bgzf_deflate_dev on torch uint8 tensors of the deflater's device.  Returns (rc, bytes written): rc 0 or ERR_CAPACITY (nothing written)."""
        n = C.c_uint64()
        rc = lib().mcx_bgzf_deflate_dev(self._h, d_text.data_ptr() if text_bytes else None, text_bytes, d_out.data_ptr(), d_out.numel() if out_cap is None else out_cap, C.byref(n))
        if rc not in (0, ERR_CAPACITY):
            _check(rc, "mcx_bgzf_deflate_dev")
        return rc, int(n.value)

    def deflate(self, text) -> bytes:
        """mcx_bgzf_deflate on host buffers: the BGZF blocks of ``text`` (no EOF block)."""
        src = np.frombuffer(bytes(text), dtype=np.uint8)
        out = np.zeros(max(self.bound(src.size), 1), dtype=np.uint8)
        n = C.c_uint64()
        _check(lib().mcx_bgzf_deflate(self._h, src.ctypes.data if src.size else None, src.size, out.ctypes.data, out.size, C.byref(n)), "mcx_bgzf_deflate")
        return out[:n.value].tobytes()

    def blocks(self) -> Tuple[int, int]:
        """mcx_bgzf_deflate_blocks: (a device pointer to n_blocks + 1 uint64 — where each block of the last deflate_dev begins in its output, the last entry its size —,
        n_blocks); the array is the deflater's and holds until its next call"""
        p, n = C.c_void_p(), C.c_uint64()
        _check(lib().mcx_bgzf_deflate_blocks(self._h, C.byref(p), C.byref(n)), "mcx_bgzf_deflate_blocks")
        return int(p.value or 0), int(n.value)

    def last_ms(self) -> float:
        """the last deflate_dev's kernels, in ms by events on the deflater's stream"""
        ms = C.c_float()
        _check(lib().mcx_bgzf_deflate_last_ms(self._h, C.byref(ms)), "mcx_bgzf_deflate_last_ms")
        return float(ms.value)


def bgzf_eof() -> bytes:
    """mcx_bgzf_eof: the empty block that ends a BGZF file"""
    out = (C.c_uint8 * 28)()
    _check(lib().mcx_bgzf_eof(out), "mcx_bgzf_eof")
    return bytes(out)


def bgzf_deflate(text, block: int = 65280, device: int = 0) -> bytes:
    """``text`` as the BGZF blocks the device makes of it (block: bytes of text per block), without the EOF block: gzip.decompress(bgzf_deflate(t) + bgzf_eof()) == t"""
    with Deflater(device) as d:
        if d.set_block(block) != 0:
            raise ValueError("a BGZF block takes 1 to 65280 bytes of text")
        return d.deflate(text)


def bgzf_inflate(path: str, device: int = 0, cap: int = 0):
    """mcx_bgzf_inflate: (the text's whole length | -1 no BGZF file | -2 a damaged member, the first min(cap, delivered) bytes of the text)."""
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_uint64()
    total = int(lib().mcx_bgzf_inflate(path.encode(), device, out.ctypes.data, cap, C.byref(n)))
    return total, out[:min(cap, n.value)].tobytes()


def gz_inflate_dev(path: str, device: int = 0, stretch_bytes: int = 0, round_stretches: int = 0, cap: int = 0):
    """mcx_gz_inflate_dev: (the text's whole length | -1 no gzip file | -2 a damaged stream, the first min(cap, delivered) bytes of the text)."""
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    n = C.c_uint64()
    total = int(lib().mcx_gz_inflate_dev(path.encode(), device, stretch_bytes, round_stretches, out.ctypes.data, cap, C.byref(n)))
    return total, out[:min(cap, n.value)].tobytes()


def gz_inflate_dev_last() -> Tuple[int, int]:
    """mcx_gz_inflate_dev_last: (rounds begun, rounds whose bytes were staged while the round before ran) of this thread's last gz_inflate_dev"""
    st = (C.c_uint64 * 2)()
    lib().mcx_gz_inflate_dev_last(C.byref(st))
    return int(st[0]), int(st[1])


def _pool_of(aln: np.ndarray, cigars):
    """(records, pool): ``cigars`` a pool the records' cigar_off point into, or a list of per-record word arrays (map_batch's form),
    which are put back to back with the records' offsets rewritten."""
    aln = np.ascontiguousarray(aln, dtype=ALN_DTYPE)
    if isinstance(cigars, np.ndarray):
        return aln, np.ascontiguousarray(cigars, dtype=np.uint32)
    aln = aln.copy()
    sizes = np.array([len(c) for c in cigars], dtype=np.int64)
    aln["cigar_off"] = np.concatenate([[0], np.cumsum(sizes)[:-1]]) if len(sizes) else 0
    pool = np.concatenate([np.asarray(c, dtype=np.uint32) for c in cigars] + [np.zeros(1, dtype=np.uint32)])
    return aln, pool


def _sam_in(bases, off, names, quals, paired, aln, pool, extras):
    """(SamIn over host arrays, what keeps them alive): the arguments of Mapper.sam_text / bam_records as mcx_sam_in"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint32)
    n = off.size - 1
    aln, pool = _pool_of(aln, pool)
    name_off = np.zeros(n + 1, dtype=np.uint32)
    name_off[1:] = np.cumsum([len(x) for x in names])
    name_buf = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8).copy()
    si = SamIn()
    si.bases, si.off, si.names, si.name_off = bases.ctypes.data, off.ctypes.data, name_buf.ctypes.data, name_off.ctypes.data
    si.aln, si.cigar, si.n_reads, si.paired = aln.ctypes.data, pool.ctypes.data, n, int(paired)
    keep = [bases, off, aln, pool, name_off, name_buf]
    if quals is not None:
        q = np.zeros(max(1, int(off[-1])), dtype=np.uint8)
        for r, b in enumerate(quals):
            b = b[:int(off[r + 1]) - int(off[r])]
            q[int(off[r]):int(off[r]) + len(b)] = np.frombuffer(b, dtype=np.uint8)
        keep.append(q)
        si.qual = q.ctypes.data
    if extras is not None:
        index = np.ascontiguousarray(extras[0], dtype=np.uint32)
        x_recs, x_pool = _pool_of(extras[1], extras[2])
        keep += [index, x_recs, x_pool]
        si.x_index, si.x_recs, si.x_cigar = index.ctypes.data, x_recs.ctypes.data, x_pool.ctypes.data
    return si, keep


def rg_parse(arg: str) -> Tuple[bytes, bytes]:
    """mcx_rg_parse: (the @RG line with real TABs and no newline, its ID) of a -rg argument in bwa mem -R's form; McxError (ERR_ARG) says why it is refused"""
    buf = C.create_string_buffer(4097)
    nb, at, n = C.c_uint64(), C.c_uint32(), C.c_uint32()
    _check(lib().mcx_rg_parse(arg.encode("latin-1") if isinstance(arg, str) else arg, buf, 4096, C.byref(nb), C.byref(at), C.byref(n)), "mcx_rg_parse")
    line = buf.raw[:nb.value]
    return line, line[at.value:at.value + n.value]


def _sam_tags(read_group, mate_tags, keep):
    """the SamTags of Mapper.sam_text / bam_records (None: both off)"""
    if read_group is None and not mate_tags:
        return None
    tg = SamTags()
    tg.mate_tags = int(bool(mate_tags))
    if read_group is not None:
        rid = np.frombuffer(rg_parse(read_group)[1] + b"\0", dtype=np.uint8).copy()
        keep.append(rid)
        tg.rg, tg.rg_len = rid.ctypes.data, rid.size - 1
    return C.pointer(tg)


def sam_header(index: "Index", read_group: Optional[str] = None) -> bytes:
    """The @PG / @SQ lines the file front end writes ahead of the first batch (mcx_sam_header); ``read_group``: with its @RG line as the last (mcx_sam_header_rg)."""
    rg = rg_parse(read_group)[0] if read_group is not None else None
    nb = C.c_uint64()
    rc = lib().mcx_sam_header_rg(index._h, rg, None, 0, C.byref(nb))
    if rc not in (0, ERR_CAPACITY):
        _check(rc, "mcx_sam_header")
    buf = C.create_string_buffer(max(1, nb.value))
    _check(lib().mcx_sam_header_rg(index._h, rg, buf, nb.value, C.byref(nb)), "mcx_sam_header")
    return buf.raw[:nb.value]


def bam_header(index: "Index", sorted: bool = False, read_group: Optional[str] = None) -> bytes:
    """The uncompressed BAM header the file front end writes (as BGZF blocks) ahead of the first batch with ``bam``: magic, sam_header's text, the contigs (mcx_bam_header);
    ``sorted``: the header of a ``sort`` run, whose text begins with @HD VN:1.6 SO:coordinate (mcx_bam_header_sorted)."""
    if read_group is not None:  # ... with the @RG line as the last line of the text (mcx_bam_header_rg)
        rg, what = rg_parse(read_group)[0], "mcx_bam_header_rg"
        call = lambda h, out, cap, nb: lib().mcx_bam_header_rg(h, rg, int(sorted), out, cap, nb)
    else:
        call, what = (lib().mcx_bam_header_sorted, "mcx_bam_header_sorted") if sorted else (lib().mcx_bam_header, "mcx_bam_header")
    nb = C.c_uint64()
    rc = call(index._h, None, 0, C.byref(nb))
    if rc not in (0, ERR_CAPACITY):
        _check(rc, what)
    buf = C.create_string_buffer(max(1, nb.value))
    _check(call(index._h, buf, nb.value, C.byref(nb)), what)
    return buf.raw[:nb.value]


def avg_advance(state, pairs: int, dist: int, n_chunks: int):
    """The trajectory's state after a round that held ``pairs`` proper pairs at the summed distance ``dist`` (in place: a list of three)."""
    st = (C.c_int64 * 3)(*[int(v) for v in state])
    lib().mcx_avg_advance(st, int(pairs), int(dist), int(n_chunks))
    state[0], state[1], state[2] = int(st[0]), int(st[1]), int(st[2])
    return state


def avg_walk(state, pairs: np.ndarray, dist: np.ndarray, want_est: bool = True):
    """mcx_avg_walk: advances state = [avgDist, pairs, distance] over the chunks; returns the per-chunk EstiDistance."""
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32)
    dist = np.ascontiguousarray(dist, dtype=np.uint32)
    st = (C.c_int64 * 3)(*[int(v) for v in state[:3]])
    est = np.zeros(pairs.size, dtype=np.int32) if want_est else None
    lib().mcx_avg_walk(st, pairs.ctypes.data, dist.ctypes.data, pairs.size, est.ctypes.data if want_est else None)
    state[0], state[1], state[2] = st[0], st[1], st[2]
    return est


def apply_ops(q: str, t: str, ops: str) -> Tuple[str, str]:
    """Gapped strings the reference's nw_alignment / ksw2_alignment would leave in s1, s2."""
    a, b, i, j = [], [], 0, 0
    for o in ops:
        if o == "M":
            a.append(q[i]); b.append(t[j]); i += 1; j += 1
        elif o == "I":
            a.append(q[i]); b.append("-"); i += 1
        else:
            a.append("-"); b.append(t[j]); j += 1
    return "".join(a), "".join(b)


def sparse_to_maps_text(sparse) -> str:
    """The text form oracle/_ref/mcref_tool 'P' and mcxo_map_files_profile write (<out>.maps):
    insert / delete / break-point maps in std::map order, then the inversion and translocation
    site lists sorted by position (stable)."""
    ins, dele, brk = {}, {}, {}
    inv, tnl = [], []
    for t, pos, v in sparse:
        if t == "I":
            ins[(pos, v)] = ins.get((pos, v), 0) + 1
        elif t == "D":
            dele[(pos, v)] = dele.get((pos, v), 0) + 1
        elif t == "B":
            brk[pos] = brk.get(pos, 0) + 1
        elif t == "V":
            inv.append((pos, v))
        else:
            tnl.append((pos, v))
    lines = []
    for name, m in (("I", ins), ("D", dele)):
        for (pos, seq) in sorted(m, key=lambda k: (k[0], k[1].encode("latin-1"))):
            lines.append(f"{name} {pos} {seq} {m[(pos, seq)]}")
    for pos in sorted(brk):
        lines.append(f"B {pos} {brk[pos]}")
    for name, lst in (("V", inv), ("T", tnl)):
        for pos, dist in sorted(lst, key=lambda k: k[0]):
            lines.append(f"{name} {pos} {dist}")
    return "".join(l + "\n" for l in lines)
