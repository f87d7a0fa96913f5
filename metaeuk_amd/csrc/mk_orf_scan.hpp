// metaeuk_amd/csrc/mk_orf_scan.hpp -- the ORF-fragment rule of `extractorfs` with orf-start-mode 1, one restatement for the kernels of
// mk_orf.hip and the host twin (mk_extract_orfs_host, mk_orf_host.cpp).
//   Orf::setSequence / findAll / findForward    M/src/commons/Orf.cpp:127-348
//   the filter of the extractorfs loop          M/src/util/extractorfs.cpp:80-89
//   TranslateNucl::translate                    M/src/commons/TranslateNucl.h:488-503
// With orf-start-mode 1 a fragment is a maximal stop-free codon run of one frame: it ENDS at a stop codon or at the last complete codon of
// the frame, and STARTS three behind the previous stop of the frame (or at the frame offset: incomplete start).  So every strand position
// decides on its own whether a fragment ends there (a short backward walk to the previous stop), and the reference's output order --
// contig, plus strand then minus strand, end position ascending across the three frames -- is the order of the position index itself.
// The filters of the rule only DROP fragments; a dropped fragment still closes its frame (findForward leaves the ORF before it tests the
// limits), so the per-position view holds for every setting:
//   frame masks     bit f - 1 of a strand's mask enables the codons at strand position = f - 1 (mod 3); the minus strand's positions are
//                   those of the reverse complement (Orf.cpp:268-273)
//   --max-gaps G    more than G gap codons between the first and the closing codon, both included (Orf.cpp:313-315, 338); a gap codon holds
//                   an N or a character without an IUPAC complement, tested on the upper-cased character (isGapOrN, Orf.cpp:195-199)
//   --min-length / --max-length   codons, the closing stop not counted (Orf.cpp:309-311, 339-340)
//   --contig-end-mode             0 keeps the fragments without a stop, 1 those with one, 2 both (extractorfs.cpp:87-89)
// The tables are a policy class `Tab` with static complement(c) / base_code(c): __constant__ arrays in the kernels, plain arrays on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>

namespace mk {

struct OrfRule {
    uint32_t min_length, max_length;       // codons (Orf::findAll's minLength / maxLength)
    uint32_t max_gaps;                     // gap codons; >= INT_MAX: no limit, and the walk does not count
    uint32_t forward_frames, reverse_frames;   // Orf::FRAME_1 | FRAME_2 | FRAME_3 of the plus and the minus strand; 0 skips the strand
                                           // (two scalars: a lane picks one by its strand without indexing the kernel arguments)
    uint32_t end_mode;                     // --contig-end-mode
    uint32_t reverse;                      // --reverse-fragments: the residues of a fragment are written back to front (reverseseq.cpp:41-47)
};
__host__ __device__ inline bool orf_rule_counts_gaps(const OrfRule &r) { return r.max_gaps < (uint32_t) INT_MAX; }

template <class Tab>
struct Strand {
    const char *seq; uint32_t len; bool minus;
    // Orf::setSequence: only 'u' becomes 't' (the second assignment of the reference wins); minus strand = complement of
    // the mirrored position, '.' -> 'N'; CHAR_MAX behind the end
    __host__ __device__ __forceinline__ char at(uint32_t i) const {
        if (i >= len) return (char) CHAR_MAX;
        char c = seq[minus ? len - 1 - i : i];
        if (c == 'u') c = 't';
        if (minus) { c = Tab::complement((unsigned char) c); if (c == '.') c = 'N'; }
        return c;
    }
};

__host__ __device__ __forceinline__ char upper_or_max(char c) { return c == (char) CHAR_MAX ? c : (char) (c & (unsigned char) ~0x20); }
__host__ __device__ __forceinline__ bool stop_codon(char c0, char c1, char c2) {          // upper-cased characters: TAA, TAG, TGA
    return c0 == 'T' && ((c1 == 'A' && (c2 == 'A' || c2 == 'G')) || (c1 == 'G' && c2 == 'A'));
}
template <class Tab>
__host__ __device__ __forceinline__ bool not_nucleotide(char upper) { return upper == 'N' || Tab::complement((unsigned char) upper) == '.'; }

template <class Tab>
__host__ __device__ __forceinline__ bool stop_at(const Strand<Tab> &S, uint32_t p) {
    const char c0 = upper_or_max(S.at(p));
    if (c0 != 'T') return false;
    return stop_codon(c0, upper_or_max(S.at(p + 1)), upper_or_max(S.at(p + 2)));
}

// the codon at p with all three characters loaded: is it a stop, does it hold a gap (the walk of a launch with a gap limit)
template <class Tab>
__host__ __device__ __forceinline__ bool stop_or_gap_at(const Strand<Tab> &S, uint32_t p, bool &gap) {
    const char c0 = upper_or_max(S.at(p)), c1 = upper_or_max(S.at(p + 1)), c2 = upper_or_max(S.at(p + 2));
    gap = not_nucleotide<Tab>(c0) || not_nucleotide<Tab>(c1) || not_nucleotide<Tab>(c2);
    return stop_codon(c0, c1, c2);
}

// fragment ending at strand position p (0 codons = none): start, length, flags (1 = incomplete start, 2 = incomplete end, 4 = minus strand).
// GAPS = the rule has a gap limit (launch-uniform): the walk then loads the whole codon and stops once the count is over the limit.
template <bool GAPS, class Tab>
__host__ __device__ __forceinline__ uint32_t fragment_at(const Strand<Tab> &S, uint32_t p, const OrfRule &R, uint32_t &from, uint32_t &flags) {
    if (!(((S.minus ? R.reverse_frames : R.forward_frames) >> (p % 3u)) & 1u)) return 0;      // frame not asked for: nothing is loaded
    if (S.len < 3 || p + 3 > S.len) return 0;                           // incomplete codon: never ends a fragment
    uint32_t gaps = 0;
    bool stop;
    if (GAPS) { bool g; stop = stop_or_gap_at(S, p, g); gaps = g ? 1u : 0u; }      // (a stop codon holds no gap)
    else stop = stop_at(S, p);
    const bool last = p + 6 > S.len;                                    // the frame's next codon is incomplete
    if (!stop && !last) return 0;
    if (R.end_mode < 2 && (stop ? 0u : 1u) == R.end_mode) return 0;     // extractorfs.cpp:87: hasIncompleteEnd == contigEndMode is skipped
    if (GAPS && gaps > R.max_gaps) return 0;
    uint32_t q = p;
    bool hasStart = false;
    while (q >= 3) {                                                    // previous stop of this frame
        if (GAPS) {
            bool g;
            if (stop_or_gap_at(S, q - 3, g)) { hasStart = true; break; }
            if (g && ++gaps > R.max_gaps) return 0;                     // dropped whatever its start is: this lane emits nothing
        } else if (stop_at(S, q - 3)) { hasStart = true; break; }
        q -= 3;
    }
    from = q;                                                           // = p % 3 when no stop precedes
    const uint32_t count = (p - from) / 3 + (stop ? 0u : 1u);
    if (count == 0 || count < R.min_length || count > R.max_length) return 0;
    flags = (hasStart ? 0u : 1u) | (stop ? 0u : 2u) | (S.minus ? 4u : 0u);
    return count;
}

// residue of the codon at strand position p: TranslateNucl::translate over the IUPAC-aware table (mk::build_translation_table), a codon with
// a lower-case character gives a lower-case residue
template <class Tab>
__host__ __device__ __forceinline__ char translate_at(const Strand<Tab> &S, uint32_t p, const char *table /* [4096] */) {
    const char n0 = S.at(p), n1 = S.at(p + 1), n2 = S.at(p + 2);
    char aa = table[256 * Tab::base_code((unsigned char) n0) + 16 * Tab::base_code((unsigned char) n1) + Tab::base_code((unsigned char) n2)];
    const bool lower = (n0 >= 'a' && n0 <= 'z') || (n1 >= 'a' && n1 <= 'z') || (n2 >= 'a' && n2 <= 'z');
    if (lower && aa >= 'A' && aa <= 'Z') aa = (char) (aa + 32);
    return aa;
}

// where residue i of an n-residue fragment goes inside the fragment
__host__ __device__ __forceinline__ uint32_t orf_residue_slot(uint32_t i, uint32_t n, uint32_t reverse) { return reverse ? n - 1u - i : i; }

}  // namespace mk
