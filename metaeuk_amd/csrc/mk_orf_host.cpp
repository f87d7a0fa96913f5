// metaeuk_amd/csrc/mk_orf_host.cpp -- the ORF-fragment producer on the host: the twin of mk_orf.hip's kernels over the same rule
// (mk_orf_scan.hpp), position by position in the kernels' order.  No GPU call: the CPU suite pins the rule with it, the GPU suite checks
// the kernels against it.
#include "mk_orf.hpp"
#include <mutex>

namespace mk {

namespace {

char hComplement[256];
uint8_t hBaseCode[256];
std::once_flag hTablesOnce;

struct HostTab {
    static inline char complement(unsigned char c) { return hComplement[c]; }
    static inline uint8_t base_code(unsigned char c) { return hBaseCode[c]; }
};

// MODE < 0: the default rule (fragment_at<GAPS>), else fragment_at_modes<MODE> -- the instance the device launches for the same rule
template <int MODE, bool GAPS>
void scan(const char *nucl, const uint64_t *offsets, uint32_t nContigs, const OrfRule &rule, const char *table, OrfHostResult &out) {
    for (uint32_t c = 0; c < nContigs; c++) {
        Strand<HostTab> S;
        S.seq = nucl + offsets[c]; S.len = (uint32_t) (offsets[c + 1] - offsets[c]);
        for (int strand = 0; strand < 2; strand++) {
            S.minus = strand == 1;
            if ((strand ? rule.reverse_frames : rule.forward_frames) == 0) continue;                      // Orf::findAll skips the strand
            for (uint32_t p = 0; p < S.len; p++) {
                uint32_t from = 0, flags = 0;
                const uint32_t n = MODE < 0 ? fragment_at<GAPS>(S, p, rule, from, flags) : fragment_at_modes<MODE>(S, p, rule, from, flags);
                if (n == 0) continue;
                if (rule.add_stop) flags |= orf_star_flags(S, from, n, flags, table);
                OrfRecord r;
                r.contig = c; r.s_from = from; r.n_codons = n; r.flags = flags;
                out.records.push_back(r);
                const uint64_t base = out.aa_off.back();
                const uint32_t lead = (flags >> 3) & 1u, res = n + orf_star_count(flags);
                out.aa.resize(base + res);
                for (uint32_t i = 0; i < res; i++)
                    out.aa[base + orf_residue_slot(i, res, rule.reverse)] = (i < lead || i - lead >= n) ? '*' : translate_at(S, from + 3u * (i - lead), table);
                out.aa_off.push_back(base + res);
            }
        }
    }
}

}  // namespace

void extract_orfs_host(const char *nucl, const uint64_t *offsets, uint32_t nContigs, const OrfRule &rule, const char *table, OrfHostResult &out) {
    std::call_once(hTablesOnce, [] { build_orf_tables(hComplement, hBaseCode); });
    out.records.clear(); out.aa.clear(); out.codes.clear();
    out.aa_off.assign(1, 0);
    if (!rule.general) {
        if (orf_rule_counts_gaps(rule)) scan<-1, true>(nucl, offsets, nContigs, rule, table, out);
        else scan<-1, false>(nucl, offsets, nContigs, rule, table, out);
    } else if (rule.start_mode == 0) scan<0, true>(nucl, offsets, nContigs, rule, table, out);
    else if (rule.start_mode == 1) scan<1, true>(nucl, offsets, nContigs, rule, table, out);
    else scan<2, true>(nucl, offsets, nContigs, rule, table, out);
    out.codes.resize(out.aa.size());
    encode(out.aa.data(), out.aa.size(), out.codes.data());
}

}  // namespace mk
