// metaeuk_amd/csrc/mk_orf_host.cpp -- the ORF-fragment producer on the host: the twin of mk_orf.hip's kernels over the same rule
// (mk_orf_scan.hpp), position by position in the kernels' order.  No GPU call: the CPU suite pins the rule with it, the GPU suite checks
// the kernels against it.
#include "mk_orf.hpp"
#include <mutex>

namespace mk {

namespace {

char hComplement[256];
uint8_t hBaseCode[256];
char hTable[4096];
std::once_flag hTablesOnce;

struct HostTab {
    static inline char complement(unsigned char c) { return hComplement[c]; }
    static inline uint8_t base_code(unsigned char c) { return hBaseCode[c]; }
};

template <bool GAPS>
void scan(const char *nucl, const uint64_t *offsets, uint32_t nContigs, const OrfRule &rule, OrfHostResult &out) {
    for (uint32_t c = 0; c < nContigs; c++) {
        Strand<HostTab> S;
        S.seq = nucl + offsets[c]; S.len = (uint32_t) (offsets[c + 1] - offsets[c]);
        for (int strand = 0; strand < 2; strand++) {
            S.minus = strand == 1;
            if ((strand ? rule.reverse_frames : rule.forward_frames) == 0) continue;                      // Orf::findAll skips the strand
            for (uint32_t p = 0; p < S.len; p++) {
                uint32_t from = 0, flags = 0;
                const uint32_t n = fragment_at<GAPS>(S, p, rule, from, flags);
                if (n == 0) continue;
                OrfRecord r;
                r.contig = c; r.s_from = from; r.n_aa = n; r.flags = flags;
                out.records.push_back(r);
                const uint64_t base = out.aa_off.back();
                out.aa.resize(base + n);
                for (uint32_t i = 0; i < n; i++) out.aa[base + orf_residue_slot(i, n, rule.reverse)] = translate_at(S, from + 3u * i, hTable);
                out.aa_off.push_back(base + n);
            }
        }
    }
}

}  // namespace

void extract_orfs_host(const char *nucl, const uint64_t *offsets, uint32_t nContigs, const OrfRule &rule, OrfHostResult &out) {
    std::call_once(hTablesOnce, [] { build_orf_tables(hComplement, hBaseCode); build_translation_table(hTable); });
    out.records.clear(); out.aa.clear(); out.codes.clear();
    out.aa_off.assign(1, 0);
    if (orf_rule_counts_gaps(rule)) scan<true>(nucl, offsets, nContigs, rule, out);
    else scan<false>(nucl, offsets, nContigs, rule, out);
    out.codes.resize(out.aa.size());
    encode(out.aa.data(), out.aa.size(), out.codes.data());
}

}  // namespace mk
