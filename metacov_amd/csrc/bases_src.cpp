// Host record source of the base counter (bases.hip): the kept records of a
// coordinate-sorted BAM cut into batches in mc_bases_add_batch's layout.  It
// stands in for the read loop under pysam's AlignmentFile.count_coverage()
// (htslib sam_itr_next + bam_get_cigar / bam_get_seq / bam_get_qual); the
// reference has no counterpart.
//
// Kept: tid >= 0, (flag & flag_filter) == 0 and mapq >= min_mapq.  Of those,
// records without SEQ (l_seq == 0) and records whose CIGAR query length
// (sum of M/I/S/=/X, the CG:B,I tag resolved) differs from l_seq are skipped
// and counted (they stay in the kept count); the rest is handed out.  A
// record handed out in front of its predecessor in (tid, pos) makes the file
// unsorted: MC_E_INVALID.
//
// The file is inflated window by window on host threads, the next window
// while the current one is walked (the pattern of scan_src.cpp).
#include <cstring>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>

#include "bgzf.h"
#include "common.h"

using namespace mc::bgzf;

struct mc_bases_src {
    std::string path;
    MappedFile mf;
    int nt = 1;
    uint32_t flag_filter = 0x704;
    int min_mapq = 0;
    std::vector<std::string> names;
    std::vector<int64_t> lens;
    int64_t n_records = 0, n_kept = 0, n_no_seq = 0, n_bad_cigar = 0;
    bool have_last = false;
    int32_t last_tid = 0, last_pos = 0;
    // the current window and the next one (inflated on `prod`)
    std::unique_ptr<uint8_t[]> buf, nbuf;
    size_t cap = 0, n = 0, o = 0, next_off = 0;
    size_t window = 256ull << 20;   // inflated bytes per window (MC_BASES_WINDOW for tests)
    size_t ncap = 0, ntotal = 0;
    bool have_header = false, last = false, nlast = false, done = false;
    std::thread prod;
    int prc = 0;
    std::string perr;
    // the batch handed out by mc_bases_src_next
    std::vector<int32_t> tid, pos, l_seq;
    std::vector<int64_t> cig_off, seq_off, qual_off;
    std::vector<uint32_t> cigar;
    std::vector<uint8_t> seq, qual;
    std::vector<uint16_t> flag;          // (mc_bases_src_flags: the strand is flag & 0x10)
    std::vector<uint8_t> mapq;           // (mc_bases_src_mapq: the record's MAPQ byte as it is)
    int64_t n_bases = 0;
    ~mc_bases_src() {
        if (prod.joinable()) prod.join();
    }
    void clear_batch() {
        tid.clear();
        pos.clear();
        l_seq.clear();
        flag.clear();
        mapq.clear();
        cig_off.assign(1, 0);
        seq_off.assign(1, 0);
        qual_off.assign(1, 0);
        cigar.clear();
        seq.clear();
        qual.clear();
        n_bases = 0;
    }
};

namespace {

constexpr size_t kCarryRoom = 1 << 20;   // room before a window for the previous one's unfinished record

// Inflates the window of BGZF blocks after s->next_off into s->nbuf (after kCarryRoom).
int produce(mc_bases_src* s) {
    std::vector<Block> blocks;
    size_t total = 0;
    while (s->next_off < s->mf.size && total < s->window) {
        const size_t b0 = blocks.size();
        if (int rc = scan_blocks(s->mf.data, s->mf.size, s->next_off, s->next_off, blocks, total)) {
            s->perr = mc::last_error();
            return rc;
        }
        s->next_off = blocks[b0].cdata + blocks[b0].clen + 8;
    }
    s->nlast = s->next_off >= s->mf.size;
    s->ntotal = total;
    if (kCarryRoom + total + 8 > s->ncap) {
        s->nbuf.reset(new (std::nothrow) uint8_t[kCarryRoom + total + 8]);
        if (!s->nbuf) {
            s->ncap = 0;
            s->perr = "cannot allocate the read window for " + s->path;
            return MC_E_IO;
        }
        s->ncap = kCarryRoom + total + 8;
    }
    if (!blocks.empty() && !inflate_blocks(s->mf.data, blocks, s->nbuf.get() + kCarryRoom, s->nt)) {
        s->perr = "BGZF inflate failed in " + s->path;
        return MC_E_IO;
    }
    return MC_OK;
}

// Moves to the next window: the unparsed tail of the current one goes in
// front of it, and the window after it starts inflating in the background.
int fill(mc_bases_src* s) {
    if (s->prod.joinable()) {
        s->prod.join();
    } else {
        s->prc = produce(s);
    }
    MC_REQUIRE(s->prc == MC_OK, s->prc, "%s", s->perr.c_str());
    const size_t carry = s->n - s->o;
    if (carry <= kCarryRoom) {
        if (carry) std::memcpy(s->nbuf.get() + kCarryRoom - carry, s->buf.get() + s->o, carry);
        std::swap(s->buf, s->nbuf);
        std::swap(s->cap, s->ncap);
        s->o = kCarryRoom - carry;
        s->n = kCarryRoom + s->ntotal;
    } else {   // (a carry longer than the room: one buffer with both)
        const size_t need = carry + s->ntotal + 8;
        std::unique_ptr<uint8_t[]> nb(new (std::nothrow) uint8_t[need]);
        MC_REQUIRE(nb, MC_E_IO, "cannot allocate %zu bytes for %s", need, s->path.c_str());
        std::memcpy(nb.get(), s->buf.get() + s->o, carry);
        std::memcpy(nb.get() + carry, s->nbuf.get() + kCarryRoom, s->ntotal);
        s->buf = std::move(nb);
        s->cap = need;
        s->o = 0;
        s->n = carry + s->ntotal;
    }
    s->last = s->nlast;
    if (!s->last) s->prod = std::thread([s] { s->prc = produce(s); });
    if (!s->have_header) {
        size_t o = 0;
        if (parse_header(s->buf.get() + s->o, s->n - s->o, s->path.c_str(), s->names, s->lens, &o) == MC_OK) {
            s->have_header = true;
            s->o += o;
        } else {
            s->names.clear();
            s->lens.clear();
            MC_REQUIRE(!s->last, MC_E_IO, "%s: no valid BAM header", s->path.c_str());
        }
    }
    return MC_OK;
}

int next_batch(mc_bases_src* s, int64_t max_reads, int64_t max_bases) {
    const int32_t n_ref = (int32_t)s->names.size();
    while ((int64_t)s->tid.size() < max_reads && s->n_bases < max_bases) {
        const uint8_t* d = s->buf.get();
        if (!s->have_header || s->o + 4 > s->n || s->o + 4 + (size_t)rdi32(d + s->o) > s->n) {
            if (s->last) {
                MC_REQUIRE(s->have_header && s->o == s->n, MC_E_IO, "%s: truncated record at the end of the file",
                           s->path.c_str());
                s->done = true;
                return MC_OK;
            }
            if (int rc = fill(s)) return rc;
            continue;
        }
        const int32_t bs = rdi32(d + s->o);
        MC_REQUIRE(bs >= 32, MC_E_IO, "%s: bad record size at byte %zu of the inflated stream", s->path.c_str(),
                   s->o);
        const uint8_t* r = d + s->o + 4;
        const uint8_t* rend = r + bs;
        const int32_t tid = rdi32(r), pos = rdi32(r + 4);
        const uint32_t l_name = r[8], mapq = r[9], n_cigar = rd16(r + 12), flag = rd16(r + 14);
        const int32_t l_seq = rdi32(r + 16);
        const uint64_t seq_at = 32ull + l_name + 4ull * n_cigar;
        const uint64_t nbytes = ((uint64_t)std::max(l_seq, 0) + 1) / 2;
        MC_REQUIRE(l_seq >= 0 && seq_at + nbytes + (uint64_t)l_seq <= (uint64_t)bs && tid >= -1 && tid < n_ref,
                   MC_E_IO, "%s: malformed record at byte %zu of the inflated stream", s->path.c_str(), s->o);
        s->o += 4 + (size_t)bs;
        ++s->n_records;
        if (tid < 0 || (flag & s->flag_filter) || (int)mapq < s->min_mapq) continue;
        ++s->n_kept;
        if (l_seq == 0) {
            ++s->n_no_seq;
            continue;
        }
        const uint8_t* cig = nullptr;
        uint32_t nc = 0;
        MC_REQUIRE(cigar_of(r, rend, &cig, &nc), MC_E_IO, "%s: malformed CIGAR in record %lld", s->path.c_str(),
                   (long long)s->n_records - 1);
        int64_t qlen = 0;
        for (uint32_t k = 0; k < nc; ++k) {
            const uint32_t cw = rd32(cig + 4 * k);
            if ((0x193u >> (cw & 0xF)) & 1u) qlen += cw >> 4;   // M I S = X
        }
        if (qlen != l_seq) {
            ++s->n_bad_cigar;
            continue;
        }
        MC_REQUIRE(pos >= 0, MC_E_IO, "%s: record %lld is placed at a negative position", s->path.c_str(),
                   (long long)s->n_records - 1);
        MC_REQUIRE(!s->have_last || s->last_tid < tid || (s->last_tid == tid && s->last_pos <= pos), MC_E_INVALID,
                   "%s: record %lld is out of order (the file must be coordinate-sorted)", s->path.c_str(),
                   (long long)s->n_records - 1);
        s->have_last = true;
        s->last_tid = tid;
        s->last_pos = pos;
        s->tid.push_back(tid);
        s->pos.push_back(pos);
        s->l_seq.push_back(l_seq);
        s->flag.push_back((uint16_t)flag);
        s->mapq.push_back((uint8_t)mapq);
        const size_t w0 = s->cigar.size();
        s->cigar.resize(w0 + nc);
        for (uint32_t k = 0; k < nc; ++k) s->cigar[w0 + k] = rd32(cig + 4 * k);
        s->cig_off.push_back((int64_t)s->cigar.size());
        s->seq.insert(s->seq.end(), r + seq_at, r + seq_at + nbytes);
        s->seq.resize((s->seq.size() + 3) & ~size_t(3), 0);   // 4-byte aligned starts
        s->seq_off.push_back((int64_t)s->seq.size());
        s->qual.insert(s->qual.end(), r + seq_at + nbytes, r + seq_at + nbytes + (size_t)l_seq);
        s->qual_off.push_back((int64_t)s->qual.size());
        s->n_bases += l_seq;
    }
    return MC_OK;
}

}  // namespace

extern "C" int mc_bases_src_open(const char* path, int n_threads, uint32_t flag_filter, int min_mapq,
                                 mc_bases_src** out) {
    MC_REQUIRE(path && out, MC_E_INVALID, "null argument");
    *out = nullptr;
    MC_REQUIRE(min_mapq >= 0 && min_mapq <= 255, MC_E_INVALID, "min_mapq %d outside 0..255", min_mapq);
    std::unique_ptr<mc_bases_src> s(new mc_bases_src());
    s->path = path;
    s->nt = n_threads_or_all(n_threads);
    s->flag_filter = flag_filter;
    s->min_mapq = min_mapq;
    if (const char* e = std::getenv("MC_BASES_WINDOW")) s->window = std::max<size_t>(1, std::strtoull(e, nullptr, 10));
    if (int rc = s->mf.open(path)) return rc;
    while (!s->have_header) {
        if (int rc = fill(s.get())) return rc;
    }
    s->clear_batch();
    *out = s.release();
    return MC_OK;
}

extern "C" int mc_bases_src_close(mc_bases_src* s) {
    delete s;
    return MC_OK;
}

extern "C" int mc_bases_src_n_targets(const mc_bases_src* s, int32_t* n) {
    MC_REQUIRE(s && n, MC_E_INVALID, "null argument");
    *n = (int32_t)s->names.size();
    return MC_OK;
}

extern "C" int mc_bases_src_target(const mc_bases_src* s, int32_t i, const char** name, int64_t* length) {
    MC_REQUIRE(s && i >= 0 && (size_t)i < s->names.size(), MC_E_INVALID, "bad target %d", i);
    if (name) *name = s->names[i].c_str();
    if (length) *length = s->lens[i];
    return MC_OK;
}

extern "C" int mc_bases_src_next(mc_bases_src* s, int64_t max_reads, int64_t max_bases, int64_t* n_out) {
    MC_REQUIRE(s && n_out && max_reads > 0 && max_bases > 0, MC_E_INVALID, "bad argument");
    s->clear_batch();
    if (!s->done) {
        if (int rc = next_batch(s, max_reads, max_bases)) return rc;
    }
    *n_out = (int64_t)s->tid.size();
    return MC_OK;
}

extern "C" int mc_bases_src_batch(const mc_bases_src* s, const int32_t** tid, const int32_t** pos,
                                  const int64_t** cig_off, const uint32_t** cigar, const int32_t** l_seq,
                                  const int64_t** seq_off, const uint8_t** seq, const int64_t** qual_off,
                                  const uint8_t** qual) {
    MC_REQUIRE(s, MC_E_INVALID, "null handle");
    if (tid) *tid = s->tid.data();
    if (pos) *pos = s->pos.data();
    if (cig_off) *cig_off = s->cig_off.data();
    if (cigar) *cigar = s->cigar.data();
    if (l_seq) *l_seq = s->l_seq.data();
    if (seq_off) *seq_off = s->seq_off.data();
    if (seq) *seq = s->seq.data();
    if (qual_off) *qual_off = s->qual_off.data();
    if (qual) *qual = s->qual.data();
    return MC_OK;
}

extern "C" int mc_bases_src_flags(const mc_bases_src* s, const uint16_t** flag) {
    MC_REQUIRE(s && flag, MC_E_INVALID, "null argument");
    *flag = s->flag.data();
    return MC_OK;
}

extern "C" int mc_bases_src_mapq(const mc_bases_src* s, const uint8_t** mapq) {
    MC_REQUIRE(s && mapq, MC_E_INVALID, "null argument");
    *mapq = s->mapq.data();
    return MC_OK;
}

extern "C" int mc_bases_src_counts(const mc_bases_src* s, int64_t* records, int64_t* kept, int64_t* no_seq,
                                   int64_t* bad_cigar) {
    MC_REQUIRE(s && records && kept && no_seq && bad_cigar, MC_E_INVALID, "null argument");
    *records = s->n_records;
    *kept = s->n_kept;
    *no_seq = s->n_no_seq;
    *bad_cigar = s->n_bad_cigar;
    return MC_OK;
}
