// The bases-mode record rule (mc::gz::rec_bases, csrc/inflate.h) over every
// truncation of one record body, for a host AddressSanitizer build
// (tests/test_bases_decode.py compiles and runs it): argv[1] is a file with
// one record body (the bytes after block_size), argv[2] n_ref.  Each cut
// [0, k) is copied into a heap block of exactly k bytes, so a read past the
// cut is a heap-buffer-overflow; the class of every cut goes to stdout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/metacov_amd.h"
#include "../metacov_amd/csrc/inflate.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<uint8_t> rec;
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, fh)) > 0;) rec.insert(rec.end(), buf, buf + n);
    std::fclose(fh);
    const int32_t n_ref = std::atoi(argv[2]);
    for (size_t k = 0; k <= rec.size(); ++k) {
        uint8_t* cut = static_cast<uint8_t*>(std::malloc(k ? k : 1));
        if (!cut) return 2;
        if (k) std::memcpy(cut, rec.data(), k);
        mc::gz::RecBases rb{};
        // (k == 0: a one-byte block stands in, and the rule is given none of it)
        const int rc = mc::gz::rec_bases(cut, cut + k, n_ref, 0x704u, 0, rb);
        if (rc == mc::gz::kRbTaken) {
            // what a caller goes on to read: every address the rule returned lies inside the cut
            const uint8_t* end = cut + k;
            unsigned sum = 0;
            for (uint32_t w = 0; w < 4 * rb.n_cigar; ++w) sum += rb.cig[w];
            for (int32_t b = 0; b < (rb.l_seq + 1) / 2; ++b) sum += rb.seq[b];
            for (int32_t b = 0; b < rb.l_seq; ++b) sum += rb.qual[b];
            if (rb.cig + 4ull * rb.n_cigar > end || rb.qual + rb.l_seq > end) return 3;
            std::printf("%d %u %u\n", rc, rb.n_cigar, sum);
        } else {
            std::printf("%d\n", rc);
        }
        std::free(cut);
    }
    return 0;
}
