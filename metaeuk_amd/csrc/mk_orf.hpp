// metaeuk_amd/csrc/mk_orf.hpp -- ORF extraction + translation on the device (extractorfs --translate)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/metaeuk_amd.h"
#include "mk_host.hpp"
#include "mk_orf_scan.hpp"

namespace mk {

// one fragment: position on its strand (s_from = first nucleotide in strand coordinates), length in codons,
// flags: 1 = incomplete start, 2 = incomplete end (no stop codon), 4 = minus strand, 8 / 16 = --add-orf-stop put a '*' before / behind
// the translated codons: the fragment has n_codons + orf_star_count(flags) residues, and its header and coordinates know codons only
struct OrfRecord { uint32_t contig; uint32_t s_from; uint32_t n_codons; uint32_t flags; };

struct OrfScanArgs {
    const char *nucl; const uint64_t *offsets; uint32_t n_contigs;
    OrfRule rule;                                                    // Orf::findAll's arguments + the filter of the extractorfs loop
    OrfRecord *records; uint64_t *aa_off;
};

struct OrfDeviceResult {
    uint64_t n_frag = 0, n_aa = 0;
    OrfRecord *records = nullptr; uint64_t *aa_off = nullptr;        // [n_frag], [n_frag + 1]
    char *aa_ascii = nullptr; uint8_t *aa_code = nullptr;            // [n_aa]
    size_t cap[4] = {0, 0, 0, 0};                                    // the four blocks come from the batch pool (mk::dev_block_alloc)
    void release();
};

// contigs (ASCII, concatenated, offsets[n+1]) already in HBM -> fragments in the reference's output order
// (`table` = mk::build_translation_table of the rule's genetic code)
int run_extract_orfs(const char *dNucl, const uint64_t *dOffsets, uint32_t nContigs, const OrfRule &rule, const char *table /* [4096] */,
                     hipStream_t stream, OrfDeviceResult &R, std::string &err);

// the same fragments on the host, no GPU call (mk_orf_host.cpp): the twin the kernels are checked against.  records / aaOff[n + 1] / aa / codes
// are what the device call downloads.
struct OrfHostResult { std::vector<OrfRecord> records; std::vector<uint64_t> aa_off; std::vector<char> aa; std::vector<uint8_t> codes; };
void extract_orfs_host(const char *nucl, const uint64_t *offsets, uint32_t nContigs, const OrfRule &rule, const char *table /* [4096] */,
                       OrfHostResult &out);

}  // namespace mk
