"""Model of the per-allele quality sums (include/metacov_amd.h, "Quality
sums"), pure Python / numpy over tests/bases_model.py, restated from the
contract and not from the library's code:

bq         bq[6][N]: the sum of the quality bytes of the bases counted into a
           channel at a position; only counted bases (those that pass
           min_baseq) add; a read with absent qualities (first byte 0xFF) is
           counted and adds 0; bq[DEL] stays 0
mq         mq[6][N]: the sum of the MAPQ bytes of the reads counted into a
           channel, DEL included; the byte as it is (255 is not special)
width      uint32, modulo 2^32
sites      depth and the base allele as bases_model.sites_model; a site iff
           depth >= min_depth and some allele i != base (of A C G T DEL) has
           a[i] >= min_count, a[i] * 10^6 >= min_ppm * depth,
           mq[i] >= min_alt_mapq * a[i] and, for i != DEL,
           bq[i] >= min_alt_baseq * a[i]
"""
import numpy as np

from tests import bases_model as bm
from tests.bases_model import A, C, G, T, DEL

QUALITY_COLUMNS = ["%s_bq" % c for c in "A C G T N".split()] + ["%s_mq" % c for c in "A C G T N DEL".split()]


def base_quals(b, i):
    """(rpos int64 [k], quality int64 [k]) of every base of read i that an
    M / = / X op aligns, in reference order; 0 for a read without qualities."""
    words = b["cigar"][int(b["cig_off"][i]):int(b["cig_off"][i + 1])]
    l, qo = int(b["l_seq"][i]), int(b["qual_off"][i])
    quals = b["qual"][qo:qo + l].astype(np.int64)
    if l > 0 and quals[0] == 0xFF:
        quals = np.zeros(l, np.int64)
    rp, q = int(b["pos"][i]), 0
    pos_out, q_out = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op in (0, 7, 8):
            pos_out.append(np.arange(rp, rp + n, dtype=np.int64))
            q_out.append(quals[q:q + n])
        if op in bm.REF_OPS:
            rp += n
        if op in bm.QUERY_OPS:
            q += n
    return np.concatenate(pos_out), np.concatenate(q_out)


def counts_events(batches, mapqs, tids, starts, ends, min_baseq=0):
    """The sums from bases_model.read_events: every event of a read adds its
    MAPQ, every event that is not DEL the quality of the base at its position
    (a read covers a reference position at most once)."""
    seg_off = bm.seg_offsets(starts, ends)
    n = int(seg_off[-1])
    total, bq, mq = (np.zeros((6, n), np.int64) for _ in range(3))
    for b, m in zip(batches, mapqs):
        assert len(m) == bm.n_reads(b)
        for i in range(bm.n_reads(b)):
            p, c = bm.read_events(b, i, min_baseq)
            bp, bqual = base_quals(b, i)
            q = np.zeros(len(p), np.int64)
            is_base = c != DEL
            at = np.searchsorted(bp, p[is_base])
            assert np.array_equal(bp[at], p[is_base])
            q[is_base] = bqual[at]
            for s in range(len(tids)):
                if int(tids[s]) != int(b["tid"][i]):
                    continue
                k = (p >= int(starts[s])) & (p < int(ends[s]))
                idx = (c[k], int(seg_off[s]) + p[k] - int(starts[s]))
                np.add.at(total, idx, 1)
                np.add.at(bq, idx, q[k])
                np.add.at(mq, idx, int(m[i]))
    return seg_off, total, bq, mq


def counts_loop(batches, mapqs, tids, starts, ends, min_baseq=0):
    """The same, as a literal per-read, per-base loop."""
    seg_off = bm.seg_offsets(starts, ends)
    n = int(seg_off[-1])
    total, bq, mq = (np.zeros((6, n), np.int64) for _ in range(3))

    def count(tid, p, ch, q, m):
        for s in range(len(tids)):
            if int(tids[s]) == tid and int(starts[s]) <= p < int(ends[s]):
                i = int(seg_off[s]) + p - int(starts[s])
                total[ch, i] += 1
                bq[ch, i] += q
                mq[ch, i] += m

    for b, mapq in zip(batches, mapqs):
        for i in range(bm.n_reads(b)):
            tid, rp, q, l, m = int(b["tid"][i]), int(b["pos"][i]), 0, int(b["l_seq"][i]), int(mapq[i])
            so, qo = int(b["seq_off"][i]), int(b["qual_off"][i])
            absent = l > 0 and int(b["qual"][qo]) == 0xFF
            for w in b["cigar"][int(b["cig_off"][i]):int(b["cig_off"][i + 1])]:
                op, k = bm.OPS[int(w) & 15] if (int(w) & 15) < 9 else "?", int(w) >> 4
                if op == "N":
                    rp += k
                    continue
                for _ in range(k):
                    if op in "M=X":
                        byte = int(b["seq"][so + q // 2])
                        code = byte & 15 if q & 1 else byte >> 4
                        ch = {1: A, 2: C, 4: G, 8: T}.get(code, bm.N)
                        qv = 0 if absent else int(b["qual"][qo + q])
                        if min_baseq <= 0 or absent or qv >= min_baseq:
                            count(tid, rp, ch, qv, m)
                        rp += 1
                        q += 1
                    elif op == "D":
                        count(tid, rp, DEL, 0, m)
                        rp += 1
                    elif op in "IS":
                        q += 1
    return seg_off, total, bq, mq


def counts_model(batches, mapqs, tids, starts, ends, min_baseq=0, loop=False):
    """(seg_off, total, bq, mq), the three uint32 [6, N] (the sums modulo
    2^32); loop: the literal per-base loop in place of the event model."""
    if isinstance(batches, dict):
        batches, mapqs = [batches], [mapqs]
    seg_off, total, bq, mq = (counts_loop if loop else counts_events)(batches, mapqs, tids, starts, ends, min_baseq)
    return seg_off, total.astype(np.uint32), (bq & 0xFFFFFFFF).astype(np.uint32), (mq & 0xFFFFFFFF).astype(np.uint32)


def sites_model(total, bq, mq, seg_off, starts, min_depth=1, min_count=1, min_ppm=0, min_alt_baseq=0, min_alt_mapq=0,
                ref=None):
    """(site_first [S + 1], site_pos int64, site_counts, site_bq, site_mq
    uint32 [n, 6]), position by position in Python integers."""
    total, bq, mq = (np.asarray(x, np.int64) for x in (total, bq, mq))
    alleles = [A, C, G, T, DEL]
    hits = []
    for p in range(total.shape[1]):
        a = [int(total[c, p]) for c in alleles]
        b = [int(bq[c, p]) for c in alleles]
        m = [int(mq[c, p]) for c in alleles]
        depth = sum(a)
        base = a.index(max(a))                                  # the first maximum: the lowest channel
        if ref is not None and int(ref[p]) < 4:
            base = int(ref[p])
        ok = any(i != base and a[i] >= min_count and a[i] * 1000000 >= min_ppm * depth and
                 m[i] >= min_alt_mapq * a[i] and (alleles[i] == DEL or b[i] >= min_alt_baseq * a[i])
                 for i in range(5))
        if depth >= min_depth and ok:
            hits.append(p)
    idx = np.array(hits, np.int64)
    first = np.searchsorted(idx, np.asarray(seg_off, np.int64)).astype(np.int64)
    pos = np.zeros(len(idx), np.int64)
    for s in range(len(starts)):
        x, y = int(first[s]), int(first[s + 1])
        pos[x:y] = idx[x:y] - int(seg_off[s]) + int(starts[s])
    return (first, pos) + tuple(v[:, idx].T.astype(np.uint32).reshape(-1, 6) for v in (total, bq, mq))


def kept_mapq(path, flag_filter=bm.FLAG_FILTER, min_mapq=0):
    """uint8 MAPQ of the records bases_model.kept_reads hands out, in its order."""
    _, _, recs = bm.read_bam(path)
    out = []
    for r in recs:
        if r["tid"] < 0 or (r["flag"] & flag_filter) or r["mapq"] < min_mapq:
            continue
        if r["l_seq"] == 0 or bm.query_length(r["cigar"]) != r["l_seq"]:
            continue
        out.append(r["mapq"])
    return np.array(out, np.uint8)


def table(name_of, rows, fasta=None):
    """The `bases --quality` table: rows of (tid, 0-based pos, six counts, six
    baseq sums, six mapq sums); eleven more columns, no DEL_bq."""
    plain = bm.table(name_of, [(t, p, c) for t, p, c, _, _ in rows], fasta).split("\n")[:-1]
    out = [plain[0] + "\t" + "\t".join(QUALITY_COLUMNS)]
    for line, (_, _, _, b, m) in zip(plain[1:], rows):
        out.append(line + "\t" + "\t".join(str(int(x)) for x in list(b)[:5] + list(m)))
    return "\n".join(out) + "\n"
