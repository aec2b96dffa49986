"""`metacov pileup` on the MI355X engine — same options and CSV as the
reference command (metacov/cli.py:35-108).

    python -m metacov_amd.cli pileup -b X.bam [-rb R.blast7 | -rc R.csv] [-o out.csv]

Differences from the reference, all outside the CSV: the BAM need not be
indexed (it is decoded whole, on the GPU by default); all regions are
reduced in one batched GPU call.  Defaults follow pysam: the pileup read cap
of 8000 (`--max-depth`, 0 = exact depths; metacov_amd.depthcap) and current
htslib's end of a read without reference-consuming ops (`--legacy-endpos`
for htslib <= 1.9).  Rows are written in input order up to the first region
the reference would fail on (unknown name, bad coordinate, empty region),
and that error is raised after them, as cli.py:85-108 does.  With `-k/--kmer-histogram` every row also
carries pileup.experimental's 13 columns (cli.py:81, :93-95; SURVEY.md §8 f):
the read side runs on host threads, the k-mer correlation against `-f` on
the GPU (metacov_amd/experimental.py).

Per-base output (no counterpart in the reference):

    python -m metacov_amd.cli depth -b X.bam [-o out.bedgraph] [-rc R.csv | -rb R.blast7]
                                    [--quantize 0:1:4:100:] [--no-zero]

writes the exact depth as bedGraph runs, run-length encoded on the GPU
(metacov_amd/runs.py); one process, no read cap.

Windowed output (no counterpart in the reference either):

    python -m metacov_amd.cli coverage -b X.bam [-o out.bed] [-rc R.csv | -rb R.blast7] [--by 500]
                                       [--thresholds 1,10,30] [--dist out.dist.txt [--dist-bins 1024]]

writes the mean depth per contig, region or fixed window, the positions at or
above each threshold, and the cumulative depth distribution, all reduced on
the GPU (metacov_amd/windows.py); one process, no read cap.

Base counts (no counterpart in the reference either):

    python -m metacov_amd.cli bases -b X.bam [-o out.tsv] [-f ref.fa] [-rc R.csv | -rb R.blast7] [--min-baseq 0]
                                    [--min-mapq 0] [--min-depth 1] [--min-count 1] [--min-frac 0.0] [--all]
                                    [--strand [--min-alt-strand 0]]
                                    [--quality [--min-alt-baseq 0] [--min-alt-mapq 0]]
                                    [--decode host|gpu]

writes `contig pos ref depth A C G T N DEL` for the variant sites, or with
`--all` for every position, counted on the GPU (metacov_amd/bases.py); one
process, no read cap, `pos` 1-based.  `--decode gpu` also decodes the BAM on
the GPU, once, and keeps the records in device memory.  `--quality` appends
the sums of the counted bases' qualities and of their reads' MAPQ per allele
(`A_bq .. N_bq A_mq .. DEL_mq`) and lets a site ask for an alternative allele
whose mean qualities reach `--min-alt-baseq` / `--min-alt-mapq`.

Consensus (no counterpart in the reference either):

    python -m metacov_amd.cli consensus -b X.bam [-o out.fa] [-f ref.fa] [-rc R.csv | -rb R.blast7] [--min-baseq 0]
                                        [--min-mapq 0] [--min-depth 1] [--min-count 1] [--call-frac 0.0] [--iupac]
                                        [--fill-ref] [--aligned] [--summary FILE] [--line-width 60]
                                        [--decode host|gpu]

writes one FASTA record per contig or region, called per position from the
same counts on the GPU: the strongest of A, C, G, T and deletion if it passes
the thresholds, else N.  It never contains inserted bases.

Diversity (no counterpart in the reference either):

    python -m metacov_amd.cli diversity -b X.bam [-o out.tsv] [--by N] [-f ref.fa] [--min-baseq 0] [--min-mapq 0]
                                        [--min-depth 5] [--min-count 2] [--min-frac 0.05]
                                        [-rc R.csv | -rb R.blast7] [--decode host|gpu]

writes per contig, region or fixed window the covered positions, the base
sum, the SNV count, the nucleotide diversity pi and, with `-f`, the consensus
and population identity to the reference (conANI, popANI), reduced on the GPU
from the same counts to one row per window (csrc/bases_div.h).

Sample comparison (no counterpart in the reference either):

    python -m metacov_amd.cli compare -b A.bam -c B.bam [-o out.tsv] [--by N] [--min-baseq 0] [--min-mapq 0]
                                      [--min-depth 5] [--min-count 2] [--min-frac 0.05]
                                      [-rc R.csv | -rb R.blast7] [--decode host|gpu]

writes per contig, region or fixed window the positions covered in each and
in both of two samples mapped to one reference, where their major alleles
differ, where they share no allele (conANI and popANI between the samples)
and the mean distance of their allele frequencies, reduced on the GPU from
both samples' counts (csrc/bases_cmp.h).

Multi-GPU (one process per GPU, SURVEY.md §8 e):

    python -m torch.distributed.run --nproc-per-node 8 -m metacov_amd.cli pileup -b X.bam ...

Contigs are split across ranks by LPT on reads and length; with `X.bam.bai`
each rank decodes only its contigs' BGZF blocks (otherwise it decodes all and
keeps its shard).  Each rank reduces the regions on its contigs; one
all-gather of the region table (RCCL; MC_DIST_BACKEND=gloo for a CPU
rehearsal) brings the rows to rank 0, which writes the same CSV.
"""
import os
import sys
import time


def _prewarm_hip():
    """`python -m metacov_amd.cli` (one process): the HIP runtime and the
    device context are initialised on a thread while the imports below run
    (the library's calls release the GIL); mc_ctx_create then finds them
    done.  MC_CLI_PREWARM=0 turns it off."""
    if os.environ.get("MC_CLI_PREWARM", "1") == "0" or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return
    argv = sys.argv[1:]
    device = 0
    if "--device" in argv[:-1]:
        try:
            device = int(argv[argv.index("--device") + 1])
        except ValueError:
            pass

    def run():
        try:
            from metacov_amd import _lib
            _lib.load().mc_runtime_init(device)
        except Exception:   # noqa: BLE001 (the real calls report it)
            pass

    import threading
    threading.Thread(target=run, name="hip-prewarm", daemon=True).start()


if __name__ == "__main__":
    _prewarm_hip()

import contextlib  # noqa: E402
import csv  # noqa: E402
import json  # noqa: E402
import logging  # noqa: E402

import click  # noqa: E402
import numpy as np  # noqa: E402

from . import bases as _bases  # noqa: E402
from . import depthcap as _depthcap
from . import experimental as _experimental
from . import regions as _regions
from . import scan as _scan
from .bam import BamFile, GpuBamFile, StreamedBam, index_stats
from .engine import REGION_STAT_DTYPE, classic_stats, numpy_std

_T_IMPORTED = time.time()    # (MC_CLI_TIMES: the end of the module imports)

logging.basicConfig(level=logging.INFO,
                    format="[%(relativeCreated)6.1f %(funcName)s]  %(message)s",
                    datefmt="%I:%M:%S")
log = logging.getLogger(__name__)


@click.group()
def main():
    """
    MetaCov estimates abundance values from the stacking depth of
    reads mapped to a reference.
    """


# ---- what the commands besides `pileup` and `scan` share: options, checks, segments ----

def _options(*options):
    """One decorator from several; --help lists them in the order given."""
    def decorate(f):
        for option in reversed(options):
            f = option(f)
        return f
    return decorate


_opt_regions = _options(
    click.option('--regionfile-blast7', '-rb', type=click.File('r'), help="Input Region file in BLAST7 format"),
    click.option('--regionfile-csv', '-rc', type=click.File('r'), help="Input Region file in CSV format"))
_opt_by = click.option('--by', type=int, default=0, metavar="N",
                       help="0 (default): one row per contig / region; N >= 16: fixed windows of N positions")
_opt_device = click.option('--device', type=int, default=0, help="HIP device ordinal")
# --device --decode --legacy-endpos of `depth` and `coverage`: the engine's decoders
_opt_engine = _options(
    _opt_device,
    click.option('--decode', type=click.Choice(['gpu', 'host']), default='gpu',
                 help="gpu (default): BGZF inflate and record parse on the device; "
                      "host: the C++ decoder on host threads"),
    click.option('--legacy-endpos', is_flag=True, default=False,
                 help="Count a mapped read without reference-consuming CIGAR ops on one column "
                      "(htslib <= 1.9 bam_endpos); default: it adds nothing (current htslib)"))


def _opt_floors(baseq_help):
    """--min-baseq (with the command's wording) and --min-mapq."""
    return _options(click.option('--min-baseq', type=click.IntRange(0), default=0, help=baseq_help),
                    click.option('--min-mapq', type=click.IntRange(0, 255), default=0,
                                 help="Use only reads of at least this mapping quality"))


def _opt_counter(decode_help="Where the BAM is decoded: on host threads, one pass per group of 2^30 positions, or "
                             "once on the GPU, the records staying in device memory (the file's reads must fit "
                             "there)"):
    """--device and --decode of the base-counter commands."""
    return _options(_opt_device, click.option('--decode', type=click.Choice(['host', 'gpu']), default='host',
                                              help=decode_help))


def _one_region_file(rb, rc):
    if rb and rc:
        raise click.BadParameter("Only one of regionfile-blast7 and regionfile-csv may be specified")


def _ppm(frac, hint):
    """A fraction option as parts per million; refused outside [0, 1] (nan fails both comparisons)."""
    if not 0.0 <= frac <= 1.0:
        raise click.BadParameter("must lie in [0, 1]", param_hint=hint)
    return int(round(frac * 1e6))


def _window_at_least(by):
    """--by of `diversity` and `compare`."""
    if by != 0 and by < _bases.DIV_MIN_WINDOW:
        raise click.BadParameter("must be 0 or at least %d" % _bases.DIV_MIN_WINDOW, param_hint="--by")


def _single_process(name):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise click.UsageError("%s runs in one process (WORLD_SIZE > 1 is not supported: "
                               "its output is not sharded)" % name)


def _select_segments(header, rb, rc):
    """The segments (header contig ids) a command works through: the regions
    of a region file up to the first failing one, else every contig whole.
    Returns (tids, starts, ends, err, from_regions); the caller raises err
    after it has written those segments, as pileup does."""
    if rb or rc:
        _, tids, starts, ends, err = resolve_regions(header, _regions.make_region_iterator(rb, rc, header))
        return tids, starts, ends, err, True
    tids = np.arange(len(header.lengths), dtype=np.int32)
    return tids, np.zeros(len(tids), np.int64), np.asarray(header.lengths, np.int64), None, False


def _log_record_counts(counts, label=None):
    """A base source's record counts (None: nothing was read), logged under the calling command's name."""
    if counts:
        log.info(("Sample %s, number" % label if label else "Number") +
                 " of records:\n  total:    {records}\n  kept:     {kept}\n  skipped, no SEQ:           {no_seq}\n"
                 "  skipped, CIGAR != l_seq:   {bad_cigar}\n".format(**counts), stacklevel=2)


@main.command()
@click.option('--bamfile', '-b', type=click.File('rb'), required=True,
              help="Input BAM file. Must be coordinate-sorted.")
@click.option('--reference-fasta', '-f', type=click.File('rb'))
@click.option('--regionfile-blast7', '-rb', type=click.File('r'),
              help="Input Region file in BLAST7 format")
@click.option('--regionfile-csv', '-rc', type=click.File('r'),
              help="Input Region file in CSV format")
@click.option('--kmer-histogram', '-k', type=click.File('r'),
              help="Kmer Histogram produced with metacov scan")
@click.option('--kmer-length', '-K', type=int, default=7,
              help="Length of k-mer")
@click.option('--outfile', '-o', type=click.File('w'), default="-",
              help="Output CSV (default STDOUT)")
@click.option('--device', type=int, default=0, help="HIP device ordinal")
@click.option('--stream/--no-stream', default=True,
              help="Decode in bounded-memory windows, feeding the GPU through pinned double "
                   "buffers (default; --no-stream decodes the whole file into host memory first)")
@click.option('--max-depth', type=click.IntRange(0), default=_depthcap.HTSLIB_MAX_DEPTH,
              metavar="N", show_default=True,
              help="htslib's pileup read cap per region query, as pysam's pileup applies it "
                   "(its default is 8000); 0: exact depths, no cap")
@click.option('--legacy-endpos', is_flag=True, default=False,
              help="Count a mapped read without reference-consuming CIGAR ops on one column "
                   "(htslib <= 1.9 bam_endpos); default: it adds nothing (current htslib)")
@click.option('--window-bytes', type=click.IntRange(0), default=0, metavar="B",
              help="Decode in windows of B inflated bytes (bounded memory); 0: --decode gpu keeps "
                   "the file resident when it fits in HBM, --stream uses 256 MiB")
@click.option('--decode', type=click.Choice(['gpu', 'host']), default='gpu',
              help="gpu (default): BGZF inflate and record parse on the device (csrc/bam_gpu.hip); "
                   "host: the C++ decoder on host threads (--stream / --no-stream)")
def pileup(bamfile, reference_fasta, regionfile_blast7, regionfile_csv,
           kmer_histogram, kmer_length, outfile, device, stream, max_depth, legacy_endpos,
           window_bytes, decode):
    """
    Compute fold coverage values
    """
    fasta = reference_fasta.name if reference_fasta else None
    if fasta:            # cli.py:59: pysam.FastaFile(...) for every run with -f
        _experimental.check_faidx(fasta)
    # cli.py:81: the histogram is read with load_kmerhist's default k_len (7)
    k_cor = _experimental.load_kmerhist(kmer_histogram) if kmer_histogram else None
    exp = (k_cor, kmer_length, fasta) if k_cor is not None else None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return pileup_distributed(bamfile.name, regionfile_blast7, regionfile_csv, outfile, exp,
                                  max_depth=max_depth, legacy_endpos=legacy_endpos, decode=decode)
    times = _PhaseTimes.start(device)
    if decode == 'gpu':
        bam = GpuBamFile(bamfile.name, device=device, window_bytes=window_bytes,
                         legacy_endpos=legacy_endpos)
    elif stream:
        bam = StreamedBam(bamfile.name, device=device, window_bytes=window_bytes,
                          legacy_endpos=legacy_endpos)
    else:
        bam = BamFile(bamfile.name, legacy_endpos=legacy_endpos)
    times.mark("decode")
    regions = _regions.make_region_iterator(regionfile_blast7, regionfile_csv, bam)
    log_counts(bam)
    write_rows(bam, regions, outfile, device=device, exp=exp, max_depth=max_depth, times=times)
    times.finish(outfile, bam)


class _PhaseTimes:
    """MC_CLI_TIMES=<path>: the single-process `pileup`'s wall-clock phases as
    JSON (scripts/cold_cli.py): process start (MC_CLI_T0, the launcher's
    clock, else the OS's process start) to the end of the imports, HIP
    runtime and device init (one ctx created and destroyed up front, so the
    decode phase holds the decode alone), decode, rows (depth, statistics,
    cap), write.  Without the variable every call is a no-op."""

    def __init__(self, path):
        self.path = path
        self.t = {}
        self.last = time.time()

    @classmethod
    def start(cls, device=0):
        path = os.environ.get("MC_CLI_TIMES")
        if not path:
            return _NoTimes()
        t0 = os.environ.get("MC_CLI_T0")
        if t0:
            t0 = float(t0)
        else:
            import psutil
            t0 = psutil.Process().create_time()
        self = cls(path)
        self.t["interpreter_and_imports_s"] = _T_IMPORTED - t0
        self.t["cli_parse_s"] = time.time() - _T_IMPORTED
        self.t0 = t0
        self.last = time.time()
        from . import _lib as L
        import ctypes
        lib = L.load()
        self.mark("library_load")
        h = ctypes.c_void_p()
        L.check(lib.mc_ctx_create(int(device), ctypes.byref(h)), lib)
        lib.mc_ctx_destroy(h)
        self.mark("hip_init")
        return self

    def mark(self, name):
        now = time.time()
        self.t[name + "_s"] = now - self.last
        self.last = now

    def finish(self, outfile, bam):
        outfile.flush()
        self.mark("write")
        self.t["total_s"] = time.time() - self.t0
        tm = getattr(bam, "timings", None)
        if tm is not None:
            self.t["decode_timings"] = {k: round(v, 3) if isinstance(v, float) else v for k, v in tm().items()}
        with open(self.path, "w") as fh:
            json.dump(self.t, fh, indent=1)


class _NoTimes:
    def mark(self, name):
        pass

    def finish(self, outfile, bam):
        pass


def log_counts(bam):
    total = bam.mapped + bam.unmapped
    log.info("Number of reads:\n  total:    {total}\n  mapped:   {mapped} ({pct}%)\n"
             "  unmapped: {unmapped}\n".format(total=total, mapped=bam.mapped,
                                                unmapped=bam.unmapped,
                                                pct=bam.mapped / total * 100 if total else 0))


def resolve_regions(bam, regions):
    """Header contig id and sorted 0-based half-open range per region, as
    cli.py:80-91, for the regions before the first one the reference fails
    on: returns (hits, tids, starts, ends, error).  The error is what the
    reference raises at that region, in its order: the region file's own
    parse error, KeyError for an unknown name (cli.py:86), ValueError from
    int() (cli.py:89), then classic()'s ValueError for a negative start or an
    empty region (pileup.py:19, a zero-size reduction).  None when every
    region resolves."""
    name2ref = {w.split()[0]: w for w in bam.references}
    ref2tid = {}
    for t, w in enumerate(bam.references):
        ref2tid.setdefault(w, t)      # first header entry, as list.index
    hits, tids, starts, ends = [], [], [], []
    err = None
    it = iter(regions)
    while True:
        try:
            hit = next(it)
        except StopIteration:
            break
        except Exception as e:        # a malformed line of the region file
            err = e
            break
        try:
            ref = name2ref[hit.sacc]
            start, end = sorted((int(hit.sstart), int(hit.send)))
            if start < 0:
                raise ValueError("start out of range (%d)" % start)
            if start == end:
                raise ValueError("zero-size array to reduction operation minimum which has "
                                 "no identity")
        except Exception as e:
            err = e
            break
        hits.append(hit)
        tids.append(ref2tid[ref])
        starts.append(start)
        ends.append(end)
    return (hits, np.array(tids, np.int32), np.array(starts, np.int64),
            np.array(ends, np.int64), err)


def compute_rows(bam, tids, starts, ends, device=0, max_depth=_depthcap.HTSLIB_MAX_DEPTH):
    """Stat rows of the regions (header contig ids) on `bam`'s engine: depth
    and statistics in one pass (fused K2) when the regions do not overlap;
    the library falls back to K2 + K3 otherwise.  max_depth: htslib's read
    cap per region query; only regions whose exact maximum could reach it
    are recomputed, together in one more engine call (metacov_amd.depthcap);
    0 / None: exact depths.  Returns (rows, std): std is numpy's own np.std
    value for the rows near a rounding tie, NaN elsewhere (engine.numpy_std)."""
    if len(tids) == 0:
        return np.zeros(0, dtype=REGION_STAT_DTYPE), np.zeros(0)
    eng = bam.engine(device, compute=False)
    local = np.asarray(bam.local_tid(tids), np.int32)
    rows = eng.compute_depth_stats(local, starts, ends)
    eng._depth_ready = True
    std = numpy_std(eng, rows, local, starts, ends)
    if max_depth:
        rows, n_cap, dropped = _depthcap.apply_cap(bam, rows, tids, starts, ends, bam.lengths,
                                                   max_depth, device, std=std)
        if n_cap:
            log.info("max_depth %d: %d regions deep enough for the pileup cap, %d reads dropped",
                     max_depth, n_cap, dropped)
    return rows, std


def experimental_results(path, exp, references, tids, starts, ends, device=0, contigs=None, extents=None):
    """pileup.experimental for every region (cli.py:93-95), or None without -k.
    contigs / extents: a distributed rank's shard, whose read table is decoded
    from those contigs' BGZF blocks only (experimental_batch)."""
    if exp is None:
        return None
    k_cor, k_len, fasta = exp
    regs = [(references[t], int(a), int(b)) for t, a, b in zip(tids, starts, ends)]
    if not regs:
        return []
    return _experimental.experimental_batch(path, k_cor, k_len, fasta, regs, device=device, contigs=contigs,
                                            extents=extents)


def write_csv(regions, rows, outfile, extra=None, std=None):
    """Rows in input order exactly as cli.py:97-108 writes them; `extra`
    (experimental_batch results) adds the -k columns, its "RCOR is ZERO"
    lines and its errors at the region where the reference meets them.
    std: numpy's std per row where given (engine.numpy_std; NaN: none)."""
    writer = None
    for i, (hit, row) in enumerate(zip(regions, rows)):
        result = classic_stats(row, None if std is None else std[i])
        if extra is not None:
            result.update(extra[i].emit(out=sys.stdout))
        if writer is None:
            writer = csv.DictWriter(outfile, fieldnames=['sacc', 'start', 'end'] + sorted(result))
            writer.writeheader()
        result.update({'sacc': hit.sacc, 'start': hit.sstart, 'end': hit.send})
        writer.writerow(result)


def write_rows(bam, regions, outfile, device=0, exp=None, max_depth=_depthcap.HTSLIB_MAX_DEPTH, times=None):
    """Resolves names like cli.py:80-91, reduces the regions in one GPU call,
    then writes rows in input order exactly as cli.py:97-108 does; the rows
    before a failing region are written before its error is raised."""
    times = times or _NoTimes()
    hits, tids, starts, ends, err = resolve_regions(bam, regions)
    times.mark("regions")
    rows, std = compute_rows(bam, tids, starts, ends, device, max_depth)
    times.mark("rows")
    extra = experimental_results(bam.filename, exp, bam.references, tids, starts, ends, device)
    if exp is not None:
        times.mark("experimental")
    write_csv(hits, rows, outfile, extra, std)
    if err is not None:
        raise err


def pileup_distributed(path, regionfile_blast7, regionfile_csv, outfile, exp=None,
                       max_depth=_depthcap.HTSLIB_MAX_DEPTH, legacy_endpos=False, decode="gpu"):
    """One rank of a multi-GPU `pileup` (launched by torch.distributed.run).
    With -k, each rank also computes the experimental columns of the regions
    on its contigs (cli.py:93-95 per region), and rank 0 gathers them with
    the table."""
    import torch
    import torch.distributed as dist
    from . import dist as mdist
    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("MC_DIST_BACKEND", "nccl")
    device = local % max(1, torch.cuda.device_count())
    if backend == "nccl":
        torch.cuda.set_device(device)
    dist.init_process_group(backend)
    coll_dev = torch.device("cuda", device) if backend == "nccl" else None
    times = {}
    t_start = time.perf_counter()
    try:
        err = region_err = None
        try:
            table_args = _pileup_shard(path, regionfile_blast7, regionfile_csv, rank, world, device,
                                       max_depth, legacy_endpos, decode, coll_dev, times)
            head, regions, tids, starts, ends, rows, std, mine, r_max, region_err, shard = table_args
            # -k: the read table of this rank's contigs only (their BGZF blocks, by
            # the BAI or rank 0's extents table), when the GPU decodes
            mine_extra = experimental_results(path, exp, head.references, tids[mine], starts[mine],
                                              ends[mine], device, *shard)
        except BaseException as e:   # every rank learns of it before the table gather
            err = e
        mdist.agree_on_error(err, device=coll_dev)
        t0 = time.perf_counter()
        table = mdist.all_gather_table(mdist.pack_rows(rows, mine, std), r_max, device=coll_dev)
        times["gather_s"] = time.perf_counter() - t0
        extra = None
        if exp is not None:          # each rank's experimental results (our own objects) to rank 0
            parts = [None] * world if rank == 0 else None
            dist.gather_object((mine.tolist(), mine_extra), parts, dst=0)
            if rank == 0:
                extra = [None] * len(regions)
                for idx, res in parts:
                    for i, r in zip(idx, res):
                        extra[i] = r
        if rank == 0:
            log_counts(head)
            write_csv(regions, mdist.unpack_rows(table, len(regions), REGION_STAT_DTYPE), outfile,
                      extra, mdist.unpack_std(table, len(regions)))
        times["total_s"] = time.perf_counter() - t_start
        log.info("rank %d/%d phases: %s", rank, world, json.dumps(times))
    finally:
        dist.destroy_process_group()
    if region_err is not None:       # every rank resolved the same regions
        raise region_err


class _Header:
    """What the ranks of a distributed pileup use of an opened BAM besides
    its reads: names, lengths and the whole file's record counts."""

    def __init__(self, references, lengths, counts):
        self.references, self.lengths = tuple(references), tuple(lengths)
        self.n_records, self.mapped, self.unmapped = counts


def _pileup_shard(path, regionfile_blast7, regionfile_csv, rank, world, device,
                  max_depth=_depthcap.HTSLIB_MAX_DEPTH, legacy_endpos=False, decode="gpu",
                  coll_dev=None, times=None):
    """This rank's part of a distributed pileup: header and regions (every
    rank; those before the first failing one, and its error), LPT contig
    shards, the rows of the regions on its contigs, and (contigs, extents)
    for its -k read table.

    Each rank decodes only its own contigs' BGZF blocks, on
    its GPU by default, located by the BAI's extents.  Without a .bai, rank 0
    decodes the whole file on its GPU, which yields the same extents table
    (mc_bam_gpu_extents: what the index would hold), and broadcasts it; the
    other ranks then decode their contigs from it.  --decode host: the C++
    host decoder (whole file without an index)."""
    from . import dist as mdist
    full = None          # rank 0 without an index: the whole-file GPU decode
    times = {} if times is None else times
    t0 = time.perf_counter()
    index = path + ".bai"
    have_index = os.path.exists(index)
    ext = None
    if have_index:       # header + per-contig counts from the index, no decode
        head = BamFile(path, contigs=[])
        reads_per, _, _ = index_stats(index, len(head.lengths))
    elif decode == "gpu":
        def whole_file():
            nonlocal full
            full = GpuBamFile(path, device=device, legacy_endpos=legacy_endpos)
            return (full.references, full.lengths, (full.n_records, full.mapped, full.unmapped),
                    full.extents())
        try:
            refs, lens, counts, ext = mdist.broadcast_result(whole_file, rank, device=coll_dev)
        except BaseException:
            if full is not None:
                full.close()
            raise
        head = _Header(refs, lens, counts)
        reads_per = ext[0]["n_mapped"]
    else:
        head = BamFile(path, legacy_endpos=legacy_endpos)
        reads_per = np.bincount(head.tid, minlength=len(head.lengths))
    times["head_s"] = time.perf_counter() - t0
    regions, tids, starts, ends, region_err = resolve_regions(
        head, _regions.make_region_iterator(regionfile_blast7, regionfile_csv, head))
    shards = mdist.lpt_shard(mdist.contig_costs(head.lengths, reads_per), world)
    owner = np.zeros(len(head.lengths), np.int64)
    for r, sh in enumerate(shards):
        owner[sh] = r
    region_rank = owner[tids] if len(tids) else np.zeros(0, np.int64)
    mine = np.nonzero(region_rank == rank)[0]
    r_max = max(1, int(np.bincount(region_rank, minlength=world).max()) if len(tids) else 1)
    rows, std = np.zeros(0, dtype=REGION_STAT_DTYPE), np.zeros(0)
    if len(mine):
        t0 = time.perf_counter()
        if full is not None:      # rank 0 keeps its shard of the whole file
            bam, full = full.restrict(shards[rank]), None
            times["decode_timings"] = {}
        elif decode == "gpu":
            bam = GpuBamFile(path, device=device, contigs=shards[rank], extents=ext,
                             legacy_endpos=legacy_endpos)
            times["decode_timings"] = {k: round(v, 3) if isinstance(v, float) else v
                                       for k, v in bam.timings().items()}
        elif have_index:
            bam = BamFile(path, contigs=shards[rank], legacy_endpos=legacy_endpos)
        else:
            bam = head.restrict(shards[rank])
        times["decode_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        try:
            rows, std = compute_rows(bam, tids[mine], starts[mine], ends[mine], device, max_depth)
        finally:
            if decode == "gpu":
                bam.close()
        times["rows_s"] = time.perf_counter() - t0
    if full is not None:
        full.close()
    # (contigs, extents) for this rank's -k read table: a contig-subset GPU decode
    shard = (shards[rank], ext) if decode == "gpu" and (have_index or ext is not None) else (None, None)
    return head, regions, tids, starts, ends, rows, std, mine, r_max, region_err, shard


DEPTH_GROUP_POSITIONS = 1 << 28     # positions per mc_runs_compute of `depth`


def depth_groups(starts, ends, limit=DEPTH_GROUP_POSITIONS):
    """Consecutive segment ranges [a, b) whose lengths total at most `limit`
    positions; a single longer segment goes alone."""
    a, total = 0, 0
    for i, n in enumerate((np.asarray(ends, np.int64) - np.asarray(starts, np.int64)).tolist()):
        if i > a and total + n > limit:
            yield a, i
            a, total = i, 0
        total += n
    if a < len(starts):
        yield a, len(starts)


def write_depth(bam, tids, starts, ends, outfile, device=0, quantize=None, zero=True):
    """The runs of the segments (header contig ids) as bedGraph lines, group
    by group, each written before the next is computed."""
    from . import runs as _runs
    edges, labels = _runs.parse_quantize(quantize) if quantize else (None, None)
    if len(tids) == 0:
        return 0
    eng = bam.engine(device)
    local = np.asarray(bam.local_tid(tids), np.int32)
    names = _bases.contig_names(bam.references)
    written = 0
    for a, b in depth_groups(starts, ends):
        r = eng.depth_runs(local[a:b], starts[a:b], ends[a:b], quantize=edges)
        r.tids = np.asarray(tids[a:b], np.int32)        # header ids, for the names
        written += _runs.write_bedgraph(r, names, outfile, zero=zero, labels=labels)
    return written


@main.command()
@click.option('--bamfile', '-b', type=click.File('rb'), required=True,
              help="Input BAM file. Must be coordinate-sorted.")
@click.option('--outfile', '-o', type=click.File('w'), default="-",
              help="Output bedGraph (default STDOUT)")
@_opt_regions
@click.option('--quantize', metavar="SPEC",
              help="Depth classes in mosdepth's form, e.g. 0:1:4:100: (classes 0:1, 1:4, 4:100, "
                   "100:inf); the value column is the class label, runs merge per class")
@click.option('--zero/--no-zero', default=True,
              help="Write zero-depth runs (default; with --quantize: runs of the first class)")
@_opt_engine
def depth(bamfile, outfile, regionfile_blast7, regionfile_csv, quantize, zero, device, decode,
          legacy_endpos):
    """
    Write per-base depth as bedGraph runs

    One line `contig start end depth` per maximal run of equal depth,
    run-length encoded on the GPU: every contig in header order over its
    whole length, or the regions of a region file in file order.  Depths are
    exact: the htslib read cap that `pileup` applies per region query is not
    applied here.  Single process only.
    """
    from . import runs as _runs
    _one_region_file(regionfile_blast7, regionfile_csv)
    if quantize:
        try:
            _runs.parse_quantize(quantize)
        except ValueError as e:
            raise click.BadParameter(str(e), param_hint="--quantize")
    _single_process("depth")
    if decode == 'gpu':
        bam = GpuBamFile(bamfile.name, device=device, legacy_endpos=legacy_endpos)
    else:
        bam = BamFile(bamfile.name, legacy_endpos=legacy_endpos)
    log_counts(bam)
    tids, starts, ends, err, _ = _select_segments(bam, regionfile_blast7, regionfile_csv)
    n = write_depth(bam, tids, starts, ends, outfile, device=device, quantize=quantize, zero=zero)
    outfile.flush()
    log.info("%d runs written", n)
    if err is not None:      # the regions before a failing one are written first, as pileup does
        raise err


HIST_GROUP_CELLS = 1 << 27          # segments x bins per mc_windows_hist of `coverage`


def write_coverage(bam, tids, starts, ends, outfile, device=0, by=0, thresholds=None, dist=None,
                   dist_bins=1024, labels=None):
    """The windows of the segments (header contig ids) as a table, group by
    group, each written before the next is computed; with `dist` also the
    cumulative depth distribution per segment (labels) and in total."""
    from . import windows as _windows
    thr = _windows.parse_thresholds(thresholds) if thresholds else []
    names = _bases.contig_names(bam.references)
    if len(tids) == 0:
        _windows.write_windows_bed(_windows.WindowCoverage([], [], [], by, thr, [0], [], []), names, outfile)
        if dist is not None:
            _windows.write_dist(np.zeros((0, dist_bins), np.int64), [], dist)
        return 0
    eng = bam.engine(device)
    local = np.asarray(bam.local_tid(tids), np.int32)
    written = 0
    hists = []
    per_call = max(1, HIST_GROUP_CELLS // dist_bins)
    for a, b in depth_groups(starts, ends):
        wc = eng.depth_windows(local[a:b], starts[a:b], ends[a:b], window=by, thresholds=thr)
        wc.tids = np.asarray(tids[a:b], np.int32)       # header ids, for the names
        written += _windows.write_windows_bed(wc, names, outfile, header=a == 0)
        if dist is not None:
            for c in range(a, b, per_call):
                d = min(b, c + per_call)
                hists.append(eng.depth_hist(local[c:d], starts[c:d], ends[c:d], n_bins=dist_bins))
    if dist is not None:
        _windows.write_dist(np.concatenate(hists), labels, dist)
    return written


@main.command()
@click.option('--bamfile', '-b', type=click.File('rb'), required=True,
              help="Input BAM file. Must be coordinate-sorted.")
@click.option('--outfile', '-o', type=click.File('w'), default="-",
              help="Output windows table (default STDOUT)")
@_opt_regions
@_opt_by
@click.option('--thresholds', metavar="LIST",
              help="Depths, e.g. 1,10,30: one more column each, the positions at or above it")
@click.option('--dist', type=click.File('w'), metavar="FILE",
              help="Also write the cumulative depth distribution: per contig in header order "
                   "(or per region, labelled name:start-end), then in total")
@click.option('--dist-bins', type=int, default=1024, metavar="N",
              help="Bins of --dist (default 1024); the last one holds every depth at or above N - 1")
@_opt_engine
def coverage(bamfile, outfile, regionfile_blast7, regionfile_csv, by, thresholds, dist, dist_bins, device,
             decode, legacy_endpos):
    """
    Write windowed coverage: mean depth, breadth, depth distribution

    One line `contig start end mean` per window, computed on the GPU: every
    contig in header order, or the regions of a region file in file order,
    whole (--by 0) or cut into windows of N positions.  --thresholds adds a
    header line and, per depth, the positions at or above it.  --dist writes
    `label depth fraction` lines: the fraction of positions with at least
    that depth.  Depths are exact: the htslib read cap that `pileup` applies
    per region query is not applied here.  Single process only.
    """
    from . import windows as _windows
    _one_region_file(regionfile_blast7, regionfile_csv)
    if by != 0 and by < _windows.MIN_WINDOW:
        raise click.BadParameter("must be 0 or at least %d (for shorter windows write `depth` runs)"
                                 % _windows.MIN_WINDOW, param_hint="--by")
    if thresholds:
        try:
            _windows.parse_thresholds(thresholds)
        except ValueError as e:
            raise click.BadParameter(str(e), param_hint="--thresholds")
    if dist_bins < 1:
        raise click.BadParameter("must be at least 1", param_hint="--dist-bins")
    _single_process("coverage")
    if decode == 'gpu':
        bam = GpuBamFile(bamfile.name, device=device, legacy_endpos=legacy_endpos)
    else:
        bam = BamFile(bamfile.name, legacy_endpos=legacy_endpos)
    log_counts(bam)
    if dist is not None and dist_bins > _windows.dims()[2]:
        raise click.BadParameter("at most %d" % _windows.dims()[2], param_hint="--dist-bins")
    labels = names = _bases.contig_names(bam.references)
    tids, starts, ends, err, from_regions = _select_segments(bam, regionfile_blast7, regionfile_csv)
    if from_regions:
        labels = ["%s:%d-%d" % (names[int(t)], a, b) for t, a, b in zip(tids, starts, ends)]
    n = write_coverage(bam, tids, starts, ends, outfile, device=device, by=by, thresholds=thresholds,
                       dist=dist, dist_bins=dist_bins, labels=labels)
    outfile.flush()
    if dist is not None:
        dist.flush()
    log.info("%d windows written", n)
    if err is not None:      # the regions before a failing one are written first, as depth does
        raise err


BASES_GROUP_POSITIONS = 1 << 30     # positions per mc_bases_begin of `bases` (24 B each on the device)


def _segment_letters(fa, name, start, end):
    """uint8 ASCII reference letters of [start, end) of contig `name`; 'N'
    where the FASTA has no base (unknown contig, past its end)."""
    out = np.full(int(end - start), ord("N"), np.uint8)
    try:
        off, n = fa.span(name, int(start), int(end))
    except KeyError:
        return out
    lead = min(max(int(start), 0), int(end)) - int(start)      # (start >= 0 here: always 0)
    out[lead:lead + n] = fa.buffer[off:off + n]
    return out


def _group_passes(paths, references, tids, starts, ends, counts, limit, device=0, decode="host", min_baseq=0,
                  min_mapq=0, fasta=None, **tracking):
    """The pass over the segments (header contig ids) that write_bases,
    write_consensus, write_diversity and write_compare share: a generator of
    (a, b, counters, letters) per group [a, b) of at most `limit` positions,
    the group before it done with.  counters: one BaseCounter per path, begun
    on the group's segments (tracking: begin's flags) and filled with the
    path's reads; decode "host": one pass over the file on host threads per
    group, "gpu": the file is decoded once on the device and every group
    reads the resident records.  letters: with `fasta` the group's reference
    letters, uint8 ASCII indexed like a plane, else None.  counts [len(paths)]
    receives the sources' record counts.  Closing the generator closes the
    counters and the sources."""
    if len(tids) == 0:
        return
    names = _bases.contig_names(references)
    fa = _experimental.FastaFile(fasta) if fasta else None
    with contextlib.ExitStack() as stack:
        bcs = [stack.enter_context(_bases.BaseCounter(len(references), device)) for _ in paths]
        srcs = [None] * len(paths)
        if decode == "gpu":
            for k, path in enumerate(paths):
                try:
                    srcs[k] = stack.enter_context(_bases.GpuBaseSource(path, device, min_mapq=min_mapq))
                except _bases._lib.MetacovError as e:
                    if "do not fit in device memory" in str(e) or "out of memory" in str(e).lower():
                        raise click.ClickException("%s: the decoded reads do not fit in the memory of device %d; "
                                                   "run with --decode host (%s)" % (path, device, e))
                    raise
        for a, b in depth_groups(starts, ends, limit):
            for k, path in enumerate(paths):
                bcs[k].begin(tids[a:b], starts[a:b], ends[a:b], min_baseq=min_baseq, **tracking)
                if srcs[k] is not None:
                    bcs[k].add_device(srcs[k])
                    counts[k] = srcs[k].counts()
                else:
                    counts[k] = bcs[k].add_bam(path, min_mapq=min_mapq)
            letters = None
            if fa is not None:
                letters = np.concatenate([_segment_letters(fa, names[int(tids[i])], starts[i], ends[i])
                                          for i in range(a, b)] + [np.zeros(0, np.uint8)])
            yield a, b, bcs, letters


def write_bases(path, references, tids, starts, ends, outfile, fasta=None, device=0, min_baseq=0, min_mapq=0,
                min_depth=1, min_count=1, min_ppm=0, every=False, decode="host", insertions=None, strand=False,
                min_alt_strand=0, quality=False, min_alt_baseq=0, min_alt_mapq=0):
    """The base-count table of the segments (header contig ids), group by
    group, each written before the next is computed.  decode "host": each
    group is one pass over the BAM on host threads; "gpu": the file is decoded
    once on the device and every group reads the resident records.
    insertions: a text file for the insertion alleles that pass the same
    thresholds with their own count (`contig pos depth count len seq`).
    strand: twelve more columns, the forward and the reverse counts; a site
    then also needs min_alt_strand reads of an alternative allele on each
    strand.  quality (not with strand): eleven more columns, the sums of the
    counted bases' quality bytes and of their reads' MAPQ per allele; a site
    then also needs an alternative allele whose sums reach min_alt_baseq and
    min_alt_mapq times its count.  Returns (lines written, the source's record
    counts)."""
    names = _bases.contig_names(references)
    if min_alt_strand and not strand:
        raise ValueError("min_alt_strand needs strand")
    if (min_alt_baseq or min_alt_mapq) and not quality:
        raise ValueError("min_alt_baseq / min_alt_mapq need quality")
    if quality and strand:
        raise ValueError("quality and strand cannot be combined")
    outfile.write(_bases.HEADER_STRAND if strand else _bases.HEADER_QUALITY if quality else _bases.HEADER)
    if insertions is not None:
        insertions.write(_bases.INSERTIONS_HEADER)
    written, counts = 0, [None]
    with contextlib.closing(_group_passes(
            [path], references, tids, starts, ends, counts, BASES_GROUP_POSITIONS, device, decode, min_baseq, min_mapq,
            fasta, insertions=insertions is not None, strand=strand, quality=quality)) as groups:
        for a, b, (bc,), letters in groups:
            seg_off = bc.seg_off
            if insertions is not None:
                _write_insertions(bc, names, tids[a:b], starts[a:b], seg_off, min_depth, min_count, min_ppm,
                                  insertions)
            if every:
                for i in range(a, b):
                    o, n = int(seg_off[i - a]), int(ends[i] - starts[i])
                    for c0 in range(0, n, _bases.GET_CHUNK):
                        c1 = min(n, c0 + _bases.GET_CHUNK)
                        planes = bc.counts(o + c0, c1 - c0)
                        bq, mq = bc.quality(o + c0, c1 - c0) if quality else (None, None)
                        written += _bases.write_sites(
                            outfile, names[int(tids[i])], np.arange(starts[i] + c0, starts[i] + c1), planes.T,
                            None if letters is None else letters[o + c0:o + c1],
                            rev=bc.counts_reverse(o + c0, c1 - c0).T if strand else None,
                            bq=bq.T if quality else None, mq=mq.T if quality else None)
            else:
                s = bc.sites(min_depth, min_count, min_ppm,
                             ref=None if letters is None else _bases.ref_codes(letters),
                             min_alt_strand=min_alt_strand, min_alt_baseq=min_alt_baseq,
                             min_alt_mapq=min_alt_mapq)
                for i in range(a, b):
                    r0, r1 = int(s.first[i - a]), int(s.first[i - a + 1])
                    idx = int(seg_off[i - a]) + (s.pos[r0:r1] - int(starts[i]))
                    written += _bases.write_sites(outfile, names[int(tids[i])], s.pos[r0:r1], s.counts[r0:r1],
                                                  None if letters is None else letters[idx],
                                                  rev=s.rev_counts[r0:r1] if strand else None,
                                                  bq=s.bq_sums[r0:r1] if quality else None,
                                                  mq=s.mq_sums[r0:r1] if quality else None)
    return written, counts[0]


def _write_insertions(bc, names, tids, starts, seg_off, min_depth, min_count, min_ppm, fh):
    """The insertion rows of the counter's current segments, in segment and
    position order; the depth column from the planes, fetched over the span of
    at most GET_CHUNK positions that a run of rows covers.  Returns the lines."""
    ins = bc.insertions(min_depth, min_count, min_ppm)
    written = 0
    for i in range(len(tids)):
        r0, r1 = int(ins.first[i]), int(ins.first[i + 1])
        while r0 < r1:
            lo = int(ins.index[r0])
            r2 = r0 + int(np.searchsorted(ins.index[r0:r1], lo + _bases.GET_CHUNK))
            hi = int(ins.index[r2 - 1]) + 1
            planes = bc.counts(lo, hi - lo).astype(np.int64)
            depth = planes[[_bases.A, _bases.C, _bases.G, _bases.T, _bases.DEL]].sum(axis=0)
            idx = ins.index[r0:r2]
            written += _bases.write_insertions(fh, names[int(tids[i])], idx - int(seg_off[i]) + int(starts[i]),
                                               depth[idx - lo], ins.count[r0:r2], ins.length[r0:r2],
                                               [ins.sequence(k) for k in range(r0, r2)])
            r0 = r2
    return written


@main.command()
@click.option('--bamfile', '-b', type=click.File('rb'), required=True,
              help="Input BAM file. Must be coordinate-sorted.")
@click.option('--outfile', '-o', type=click.File('w'), default="-",
              help="Output table (default STDOUT)")
@click.option('--reference-fasta', '-f', type=click.File('rb'),
              help="Reference FASTA (plain or gzip): fills the ref column and makes the reference base "
                   "the base allele")
@click.option('--insertions', type=click.File('w'), metavar="FILE",
              help="Also write the insertion alleles `contig pos depth count len seq` (pos: the base before "
                   "the inserted ones; seq `*`: longer than 32 or with an ambiguity code) that pass "
                   "--min-depth, --min-count and --min-frac with their own count")
@_opt_regions
@_opt_floors("Count only bases of at least this quality (deletions always count)")
@click.option('--min-depth', type=click.IntRange(0), default=1,
              help="A site needs A + C + G + T + DEL of at least this")
@click.option('--min-count', type=click.IntRange(0), default=1,
              help="A site needs this many reads on its strongest non-base allele")
@click.option('--min-frac', type=float, default=0.0,
              help="A site needs this fraction (0..1) of its depth on that allele")
@click.option('--all', 'every', is_flag=True, default=False,
              help="Write every position of the regions, not only the sites")
@click.option('--strand', is_flag=True, default=False,
              help="Also write each count per strand: twelve more columns, `A_fwd .. DEL_fwd A_rev .. DEL_rev` "
                   "(reverse: reads with flag 0x10)")
@click.option('--min-alt-strand', type=click.IntRange(0), default=0,
              help="A site needs an allele besides the base allele that passes --min-count and --min-frac and "
                   "is seen this many times on each strand (needs --strand)")
@click.option('--quality', is_flag=True, default=False,
              help="Also write the evidence behind each count: eleven more columns of exact sums, "
                   "`A_bq .. N_bq` (quality bytes of the counted bases) and `A_mq .. DEL_mq` (MAPQ of their reads); "
                   "not with --strand")
@click.option('--min-alt-baseq', type=click.IntRange(0, 255), default=0,
              help="A site needs an allele besides the base allele that passes --min-count and --min-frac and "
                   "whose mean base quality is at least this (a deletion is exempt; needs --quality)")
@click.option('--min-alt-mapq', type=click.IntRange(0, 255), default=0,
              help="... and whose reads' mean MAPQ is at least this (needs --quality)")
@_opt_counter()
def bases(bamfile, outfile, reference_fasta, insertions, regionfile_blast7, regionfile_csv, min_baseq, min_mapq,
          min_depth, min_count, min_frac, every, strand, min_alt_strand, quality, min_alt_baseq, min_alt_mapq, device,
          decode):
    """
    Write per-position base counts and variant sites

    One line `contig pos ref depth A C G T N DEL` per site: a position whose
    strongest allele besides the base allele (the reference base with -f,
    else the most frequent allele) passes --min-count and --min-frac at a
    depth of at least --min-depth; with --all every position of the regions.
    --strand adds the counts per strand, --min-alt-strand K keeps the sites
    whose alternative allele is seen K times on both strands.  --quality
    adds the quality and MAPQ sums per allele, --min-alt-baseq / --min-alt-mapq
    keep the sites whose alternative allele reaches those means.
    pos is 1-based, as in mpileup and VCF; ref is `.` without -f.  Every
    contig in header order, or the regions of a region file in file order.
    Counted on the GPU; single process only.
    """
    _one_region_file(regionfile_blast7, regionfile_csv)
    min_ppm = _ppm(min_frac, "--min-frac")
    if min_alt_strand and not strand:
        raise click.UsageError("--min-alt-strand needs --strand")
    if min_alt_baseq and not quality:
        raise click.UsageError("--min-alt-baseq needs --quality")
    if min_alt_mapq and not quality:
        raise click.UsageError("--min-alt-mapq needs --quality")
    if quality and strand:
        raise click.UsageError("--quality and --strand cannot be combined")
    _single_process("bases")
    # (read by experimental.FastaFile as `pileup -f -k` and `scan -f` read theirs: plain or gzip.  `pileup`
    # also fails where pysam's faidx would, to match the reference; `bases` has no reference to match)
    fasta = reference_fasta.name if reference_fasta else None
    with _bases.BaseSource(bamfile.name) as head:
        references = list(head.references)
    tids, starts, ends, err, _ = _select_segments(head, regionfile_blast7, regionfile_csv)
    n, counts = write_bases(bamfile.name, references, tids, starts, ends, outfile, fasta=fasta, device=device,
                            min_baseq=min_baseq, min_mapq=min_mapq, min_depth=min_depth, min_count=min_count,
                            min_ppm=min_ppm, every=every, decode=decode, insertions=insertions, strand=strand,
                            min_alt_strand=min_alt_strand, quality=quality, min_alt_baseq=min_alt_baseq,
                            min_alt_mapq=min_alt_mapq)
    outfile.flush()
    if insertions is not None:
        insertions.flush()
    _log_record_counts(counts)
    log.info("%d lines written", n)
    if err is not None:      # the regions before a failing one are written first, as pileup does
        raise err


def write_consensus(path, references, tids, starts, ends, labels, outfile, fasta=None, device=0, min_baseq=0,
                    min_mapq=0, min_depth=1, min_count=1, call_ppm=0, iupac=False, fill_ref=False, aligned=False,
                    summary=None, line_width=60, decode="host", insertions=False):
    """One FASTA record per segment (header contig ids, record names
    `labels`), group by group as write_bases does it, each written before the
    next is computed; `summary`: also the per-segment table.  insertions: the
    called insertion alleles are part of the letters (not with aligned) and
    the table has two more columns.  Returns (records written, the source's
    record counts)."""
    if insertions and aligned:
        raise ValueError("insertions has no place in the aligned output")
    names = _bases.contig_names(references)
    if summary is not None:
        summary.write(_bases.SUMMARY_HEADER_INS if insertions else _bases.SUMMARY_HEADER)
    counts = [None]
    with contextlib.closing(_group_passes(
            [path], references, tids, starts, ends, counts, BASES_GROUP_POSITIONS, device, decode, min_baseq, min_mapq,
            fasta, insertions=insertions)) as groups:
        for a, b, (bc,), letters in groups:
            cons = bc.consensus(min_depth, min_count, call_ppm, iupac, fill_ref,
                                None if letters is None else _bases.ref_codes(letters), insertions=insertions)
            for i in range(a, b):
                _bases.write_fasta(outfile, labels[i], cons.aligned(i - a) if aligned else cons.compact(i - a),
                                   line_width)
            if summary is not None:
                _bases.write_consensus_summary(summary, [names[int(t)] for t in tids[a:b]], starts[a:b], ends[a:b],
                                               cons.summary, header=False, inserted=cons.inserted)
    return len(tids), counts[0]


@main.command()
@click.option('--bamfile', '-b', type=click.File('rb'), required=True,
              help="Input BAM file. Must be coordinate-sorted.")
@click.option('--outfile', '-o', type=click.File('w'), default="-",
              help="Output FASTA (default STDOUT)")
@click.option('--reference-fasta', '-f', type=click.File('rb'),
              help="Reference FASTA (plain or gzip): counts the differences for --summary and serves --fill-ref")
@_opt_regions
@_opt_floors("Count only bases of at least this quality (deletions always count)")
@click.option('--min-depth', type=click.IntRange(0), default=1, show_default=True,
              help="Below this A + C + G + T + DEL a position is N (or the reference base with --fill-ref)")
@click.option('--min-count', type=click.IntRange(0), default=1, show_default=True,
              help="A called allele needs this many reads")
@click.option('--call-frac', type=float, default=0.0, show_default=True,
              help="A called allele needs this fraction (0..1) of the depth")
@click.option('--iupac', is_flag=True, default=False,
              help="Where two to four bases pass --min-count and --call-frac, write their IUPAC code")
@click.option('--fill-ref', is_flag=True, default=False,
              help="Write the reference base in lower case where the depth is below --min-depth (needs -f)")
@click.option('--aligned', is_flag=True, default=False,
              help="Keep deleted positions as `-`: one letter per reference position, reference coordinates")
@click.option('--insertions', is_flag=True, default=False,
              help="Write the called insertion (per position the most frequent one of at most 32 bases, if it "
                   "passes --min-count and --call-frac) behind its position's letter; not with --aligned")
@click.option('--summary', type=click.File('w'), metavar="FILE",
              help="Also write `contig start end positions called ambiguous nocall low deleted differs length` "
                   "per record (with --insertions two more columns: insertions, inserted)")
@click.option('--line-width', type=click.IntRange(0), default=60, show_default=True,
              help="Letters per FASTA line; 0: no wrap")
@_opt_counter()
def consensus(bamfile, outfile, reference_fasta, regionfile_blast7, regionfile_csv, min_baseq, min_mapq, min_depth,
              min_count, call_frac, iupac, fill_ref, aligned, insertions, summary, line_width, device, decode):
    """
    Write the consensus sequence of the reads as FASTA

    One record per contig in header order (named by the contig id), or per
    region of a region file in file order (named `name:START-END`, 1-based
    inclusive).  Per position the allele with the highest count among A, C, G,
    T and deletion is called if it passes --min-count and --call-frac; a
    called deletion is left out (or `-` with --aligned), anything else is N.
    Without --insertions the consensus never contains inserted bases; with
    it the most frequent insertion after a position, if it passes the same two
    thresholds, follows that position's letter.  Called on the GPU; single
    process only.
    """
    _one_region_file(regionfile_blast7, regionfile_csv)
    call_ppm = _ppm(call_frac, "--call-frac")
    if fill_ref and not reference_fasta:
        raise click.BadParameter("needs a reference (-f)", param_hint="--fill-ref")
    if insertions and aligned:
        raise click.BadParameter("the aligned output has one letter per reference position and no place for "
                                 "inserted bases", param_hint="--insertions")
    _single_process("consensus")
    fasta = reference_fasta.name if reference_fasta else None
    with _bases.BaseSource(bamfile.name) as head:
        references = list(head.references)
    labels = names = _bases.contig_names(references)
    tids, starts, ends, err, from_regions = _select_segments(head, regionfile_blast7, regionfile_csv)
    if from_regions:
        labels = ["%s:%d-%d" % (names[int(t)], a + 1, b) for t, a, b in zip(tids, starts, ends)]
    n, counts = write_consensus(bamfile.name, references, tids, starts, ends, labels, outfile, fasta=fasta,
                                device=device, min_baseq=min_baseq, min_mapq=min_mapq, min_depth=min_depth,
                                min_count=min_count, call_ppm=call_ppm, iupac=iupac, fill_ref=fill_ref,
                                aligned=aligned, summary=summary, line_width=line_width, decode=decode,
                                insertions=insertions)
    outfile.flush()
    if summary is not None:
        summary.flush()
    _log_record_counts(counts)
    log.info("%d sequences written", n)
    if err is not None:      # the regions before a failing one are written first, as pileup does
        raise err


def write_diversity(path, references, tids, starts, ends, outfile, fasta=None, device=0, by=0, min_baseq=0,
                    min_mapq=0, min_depth=5, min_count=2, min_ppm=50000, decode="host"):
    """The diversity table of the segments (header contig ids), group by group
    as write_bases does it, each written before the next is computed: one line
    per segment, or per window of `by` positions.  Returns (lines written, the
    source's record counts)."""
    names = _bases.contig_names(references)
    outfile.write(_bases.DIVERSITY_HEADER)
    written, counts = 0, [None]
    with contextlib.closing(_group_passes(
            [path], references, tids, starts, ends, counts, BASES_GROUP_POSITIONS, device, decode, min_baseq, min_mapq,
            fasta)) as groups:
        for a, b, (bc,), letters in groups:
            div = bc.diversity(by, min_depth, min_count, min_ppm,
                               None if letters is None else _bases.ref_codes(letters))
            written += _bases.write_diversity(outfile, [names[int(t)] for t in tids[a:b]], starts[a:b], div,
                                              header=False)
    return written, counts[0]


@main.command()
@click.option('--bamfile', '-b', type=click.File('rb'), required=True,
              help="Input BAM file. Must be coordinate-sorted.")
@click.option('--outfile', '-o', type=click.File('w'), default="-",
              help="Output table (default STDOUT)")
@_opt_by
@click.option('--reference-fasta', '-f', type=click.File('rb'),
              help="Reference FASTA (plain or gzip): fills compared, con_diff, pop_diff and the two identities")
@_opt_floors("Count only bases of at least this quality")
@click.option('--min-depth', type=click.IntRange(0), default=5, show_default=True,
              help="A position is covered with A + C + G + T of at least this (never below 2)")
@click.option('--min-count', type=click.IntRange(0), default=2, show_default=True,
              help="An allele is present in the population with this many reads ...")
@click.option('--min-frac', type=float, default=0.05, show_default=True,
              help="... and this fraction (0..1) of the position's bases")
@_opt_regions
@_opt_counter()
def diversity(bamfile, outfile, by, reference_fasta, min_baseq, min_mapq, min_depth, min_count, min_frac,
              regionfile_blast7, regionfile_csv, device, decode):
    """
    Write windowed nucleotide diversity, SNV counts and identity to the reference

    One line `contig start end positions covered bases snv pi compared
    con_diff pop_diff con_ani pop_ani` per contig in header order, or per
    region of a region file in file order, whole (--by 0) or cut into windows
    of N positions.  covered: positions with at least --min-depth bases; snv:
    covered positions whose second allele passes --min-count and --min-frac;
    pi: the mean unbiased pairwise diversity of the covered positions.  With
    -f, con_ani is the share of the covered positions whose major allele is
    the reference base, pop_ani the share where the reference base is the
    major allele or passes the two thresholds; without it both are NA.
    Deletions are not bases here.  Reduced on the GPU; single process only.
    """
    _one_region_file(regionfile_blast7, regionfile_csv)
    _window_at_least(by)
    min_ppm = _ppm(min_frac, "--min-frac")
    _single_process("diversity")
    fasta = reference_fasta.name if reference_fasta else None
    with _bases.BaseSource(bamfile.name) as head:
        references = list(head.references)
    tids, starts, ends, err, _ = _select_segments(head, regionfile_blast7, regionfile_csv)
    n, counts = write_diversity(bamfile.name, references, tids, starts, ends, outfile, fasta=fasta, device=device,
                                by=by, min_baseq=min_baseq, min_mapq=min_mapq, min_depth=min_depth,
                                min_count=min_count, min_ppm=min_ppm, decode=decode)
    outfile.flush()
    _log_record_counts(counts)
    log.info("%d windows written", n)
    if err is not None:      # the regions before a failing one are written first, as pileup does
        raise err


# positions per mc_bases_begin of `compare`: two handles' planes, 2 x 24 B per position on the device (derived
# from the plane layout, not measured), cost what one `bases` group does
COMPARE_GROUP_POSITIONS = 1 << 29


def write_compare(path_a, path_b, references, tids, starts, ends, outfile, device=0, by=0, min_baseq=0, min_mapq=0,
                  min_depth=5, min_count=2, min_ppm=50000, decode="host"):
    """The comparison table of two BAMs with one header over the segments,
    group by group as write_diversity does it, each written before the next is
    computed: one line per segment, or per window of `by` positions.  Returns
    (lines written, the record counts of the two sources)."""
    names = _bases.contig_names(references)
    outfile.write(_bases.COMPARE_HEADER)
    written, counts = 0, [None, None]
    with contextlib.closing(_group_passes(
            [path_a, path_b], references, tids, starts, ends, counts, COMPARE_GROUP_POSITIONS, device, decode,
            min_baseq, min_mapq)) as groups:
        for a, b, bcs, _ in groups:
            cmp = bcs[0].compare(bcs[1], by, min_depth, min_count, min_ppm)
            written += _bases.write_compare(outfile, [names[int(t)] for t in tids[a:b]], starts[a:b], cmp,
                                            header=False)
    return written, counts


@main.command()
@click.option('--bamfile', '-b', type=click.File('rb'), required=True,
              help="Sample A: input BAM file. Must be coordinate-sorted.")
@click.option('--compare-bamfile', '-c', type=click.File('rb'), required=True,
              help="Sample B: a BAM file with the same reference names and lengths in the same order.")
@click.option('--outfile', '-o', type=click.File('w'), default="-",
              help="Output table (default STDOUT)")
@_opt_by
@_opt_floors("Count only bases of at least this quality")
@click.option('--min-depth', type=click.IntRange(0), default=5, show_default=True,
              help="A position is covered in a sample with A + C + G + T of at least this (never below 2)")
@click.option('--min-count', type=click.IntRange(0), default=2, show_default=True,
              help="An allele is present in a sample with this many reads ...")
@click.option('--min-frac', type=float, default=0.05, show_default=True,
              help="... and this fraction (0..1) of that sample's bases at the position")
@_opt_regions
@_opt_counter("Where the BAMs are decoded: on host threads, one pass per group of 2^29 positions, or once each "
              "on the GPU, the records staying in device memory (both files' reads must fit there)")
def compare(bamfile, compare_bamfile, outfile, by, min_baseq, min_mapq, min_depth, min_count, min_frac,
            regionfile_blast7, regionfile_csv, device, decode):
    """
    Compare two samples mapped to one reference: windowed conANI / popANI between them

    One line `contig start end positions covered_a covered_b compared
    con_diff pop_diff snv con_ani pop_ani af_dist` per contig in header order,
    or per region of a region file in file order, whole (--by 0) or cut into
    windows of N positions.  compared: positions with at least --min-depth
    bases in both samples; con_diff: of those, the major alleles differ;
    pop_diff: no allele is present in both samples (an allele is present in a
    sample as its major allele or by --min-count and --min-frac); snv: a
    second allele passes the thresholds in either sample; af_dist: the mean
    total-variation distance of the allele frequencies.  Deletions are not
    bases here.  Reduced on the GPU from both samples' counts; single process
    only.
    """
    _one_region_file(regionfile_blast7, regionfile_csv)
    _window_at_least(by)
    min_ppm = _ppm(min_frac, "--min-frac")
    _single_process("compare")
    with _bases.BaseSource(bamfile.name) as head, _bases.BaseSource(compare_bamfile.name) as other:
        references = list(head.references)
        diff = _bases.same_references(bamfile.name, references, list(head.lengths), compare_bamfile.name,
                                      list(other.references), list(other.lengths))
    if diff:
        raise click.ClickException("the two files do not share one reference: " + diff)
    tids, starts, ends, err, _ = _select_segments(head, regionfile_blast7, regionfile_csv)
    n, counts = write_compare(bamfile.name, compare_bamfile.name, references, tids, starts, ends, outfile,
                              device=device, by=by, min_baseq=min_baseq, min_mapq=min_mapq, min_depth=min_depth,
                              min_count=min_count, min_ppm=min_ppm, decode=decode)
    outfile.flush()
    for label, c in zip(("A", "B"), counts):
        _log_record_counts(c, label)
    log.info("%d windows written", n)
    if err is not None:      # the regions before a failing one are written first, as pileup does
        raise err


@main.command()
@click.option("--readfile-type", "-t",
              type=click.Choice(['bam', 'fq']),
              help="Override filename based detection of readfile type.")
@click.option("--max-reads", "-m",
              type=click.IntRange(1), metavar="N",
              help="Only consider the first N reads.")
@click.option("--group-by", "-g",
              type=click.Choice(_scan.Flags.keys()), multiple=True, metavar="FLAG",
              help="Group output by BAM flag. May be specified multiple times. "
              "FLAG can be one of {}".format(list(_scan.Flags.keys())))
@click.option('--reference-fasta', '-f',
              type=click.File('rb'), metavar="FILE",
              help="Fasta file reads where mapped to. Required for boffset."
              " File may be bgzip'ed, but not gzip'ed.")
@click.option("--out-basehist", "-b",
              type=click.File("w", lazy=False), metavar="FILE",
              help="Compute histogram of base counts by position in read.")
@click.option('--boffset', '-bo',
              type=click.IntRange(0, 200), default=0, metavar="N", show_default=True,
              help="Include N bases prior to read start in base histogram. "
              "Requires reference fasta file.")
@click.option("--out-kmerhist", "-o",
              type=click.File("w", lazy=False), metavar="FILE",
              help="Compute histogram of kmers in reads")
@click.option("-k",
              type=click.IntRange(2, 12), default=7, metavar="N", show_default=True,
              help="Length of kmers")
@click.option("--step", "-s",
              type=click.IntRange(1, 100), default=7, metavar="N", show_default=True,
              help="Step between sampled kmers")
@click.option("--offset", "-O",
              type=click.IntRange(-100, 100), default=0, metavar="N", show_default=True,
              help="Offset of first sampled kmer")
@click.option("--number", "-n",
              type=click.IntRange(1, 100), default=8, metavar="N", show_default=True,
              help="Numer of sampled kmers")
@click.option('--out-mirrorhist', '-M',
              type=click.File('w', lazy=False), metavar="FILE",
              help="Compute histogram of mismatches against palindrome")
@click.option('--mirror-offset', '-MO',
              type=click.IntRange(-100, 100), default=4, metavar="N", show_default=True,
              help="Offset of palindrome center from read start")
@click.option('--mirror-length', '-Ml',
              type=click.IntRange(1, 50), default=10, metavar="N", show_default=True,
              help="Palindrome length is 2N+1")
@click.option('--out-isizehist', '-I',
              type=click.File('w', lazy=False), metavar="FILE",
              help="Compute histogram of insert sizes.")
@click.option('--device', type=int, default=0, help="HIP device ordinal")
@click.argument("readfile", nargs=-1, required=True)
def scan(readfile, readfile_type, out_basehist, boffset, out_kmerhist,
         k, number, step, offset, max_reads, reference_fasta,
         out_mirrorhist, mirror_offset, mirror_length,
         out_isizehist, group_by, device):
    """
    Gather read statistics
    """
    # reference metacov/cli.py:162-285: same options, checks and CSV files;
    # the histograms run on the GPU (metacov_amd/scan.py)
    if not readfile_type:
        for ext, ft in {'.bam': 'bam', '.sam': 'bam', '.fq': 'fq', '.fq.gz': 'fq',
                        '.fastq': 'fq', '.fastq.gz': 'fq'}.items():
            if readfile[0].endswith(ext):
                readfile_type = ft
                break
    if not readfile_type:
        raise click.UsageError("Couldn't guess input format. Please supply -t")
    if readfile_type != 'fq' and len(readfile) > 1:
        raise click.UsageError("Multiple input files only supported for fastq")
    if len(readfile) > 2:
        raise click.UsageError("At most two fastq files allowed (fwd and rev)")
    if readfile_type != 'bam' and reference_fasta:
        raise click.UsageError("Reference fasta can only be used with mapped (bam/sam) reads")

    from . import pyfq
    fasta = None
    if readfile_type == 'bam':
        infile = readfile[0]
        if os.path.exists(infile + ".bai"):
            head = BamFile(infile, contigs=[])
            mapped, unmapped, nocoor = index_stats(infile + ".bai", len(head.lengths))
            mapped, unmapped = int(mapped.sum()), int(unmapped.sum()) + nocoor
            log.info("mapped = {}, unmapped = {}, total = {}".format(
                mapped, unmapped, mapped + unmapped))
        if reference_fasta:
            fasta = reference_fasta.name
    else:
        infile = (pyfq.FastQFilePair(readfile[0], readfile[1]) if len(readfile) > 1
                  else pyfq.FastQFile(readfile[0]))

    counters = []
    if out_basehist:
        counters.append(_scan.BaseHist(boffset))
    if out_kmerhist:
        counters.append(_scan.KmerHist(k, number, step, offset))
    if out_mirrorhist:
        counters.append(_scan.MirrorHist(mirror_offset, mirror_length))
    if out_isizehist:
        counters.append(_scan.IsizeHist())
    counters = _scan.ByFlag(counters, [_scan.Flags[flag] for flag in group_by])

    nreads = _scan.scan_reads(infile, fasta, counters, maxreads=max_reads or 0, device=device)
    log.info("Processed {} reads".format(nreads))

    # the reference's output index sequence, including the missing
    # `n = n + 1` after the k-mer table (cli.py:266-285)
    n = 0
    if out_basehist:
        csv.writer(out_basehist).writerows(counters.get_rows(n))
        n = n + 1
    if out_kmerhist:
        csv.writer(out_kmerhist).writerows(counters.get_rows(n))
    if out_mirrorhist:
        csv.writer(out_mirrorhist).writerows(counters.get_rows(n))
        n = n + 1
    if out_isizehist:
        csv.writer(out_isizehist).writerows(counters.get_rows(n))
        n = n + 1


def run_and_exit():
    """`python -m metacov_amd.cli ...`: the command, then the process ends
    without tearing down what it leaves in HBM.  The outputs are closed and
    the standard streams flushed first; then os._exit skips Python's object
    teardown and the HIP runtime's destructors (the decode's buffers, ~0.13 s
    after a 5.2 GB BAM: profiles/r06/r06d_cold_cli.json) — the driver
    reclaims the device memory of an exiting process.  MC_FAST_EXIT=0: the
    ordinary exit."""
    if os.environ.get("MC_FAST_EXIT", "1") == "0":
        sys.exit(main())
    import traceback
    try:
        rc = main(standalone_mode=False)
        rc = rc if isinstance(rc, int) else 0
    except click.exceptions.ClickException as e:
        e.show()
        rc = e.exit_code
    except click.exceptions.Abort:
        print("Aborted!", file=sys.stderr)
        rc = 1
    except SystemExit as e:
        rc = e.code if isinstance(e.code, int) else (0 if e.code is None else 1)
        if e.code is not None and not isinstance(e.code, int):
            print(e.code, file=sys.stderr)
    except BaseException:   # noqa: BLE001 - printed as the interpreter would, then the same status
        traceback.print_exc()
        rc = 1
    logging.shutdown()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(rc)


if __name__ == "__main__":
    run_and_exit()
