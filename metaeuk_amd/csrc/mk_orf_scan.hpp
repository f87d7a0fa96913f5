// metaeuk_amd/csrc/mk_orf_scan.hpp -- the ORF-fragment rule of `extractorfs`, one restatement for the kernels of mk_orf.hip and the host
// twin (mk_extract_orfs_host, mk_orf_host.cpp).
//   Orf::Orf / setSequence / findAll / findForward    M/src/commons/Orf.cpp:55-96, 127-348
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
// The above is the DEFAULT rule (genetic code 1, orf-start-mode 1, no --add-orf-stop): fragment_at, whose stop test is spelled out.  Every
// other genetic code or start mode goes through fragment_at_modes further down, where the rule for them is written out.
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
    // ---- genetic code, start modes, --add-orf-stop (fragment_at_modes; all launch-uniform, so they stay in scalar registers)
    uint32_t general;                      // 0: the default rule (fragment_at), 1: fragment_at_modes
    uint32_t start_mode;                   // --orf-start-mode: 0 start to stop, 1 any to stop, 2 last start to stop
    uint32_t contig_start_mode;            // --contig-start-mode: 0 keeps the fragments with an incomplete start, 1 those with a complete one, 2 both
    uint32_t add_stop;                     // --add-orf-stop: '*' before a complete start and behind a complete end (translatenucs.cpp:57-102)
    uint64_t stop_mask, start_mask;        // bit 16 a + 4 b + c (A = 0, C = 1, G = 2, T = 3) = codon abc is a stop / a start codon of the code
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

// ---- every genetic code, every start mode (Orf.cpp:55-96, 283-345) ----
// Stops and starts are two sets of plain codons (mk::orf_code_masks): the reference compares the three upper-cased characters with the
// codons of TranslateNucl::getStopCodons() / getStartCodons() (or ATG alone), so a codon with a character outside ACGT -- TAR, NNN, UAA with
// a capital U -- is neither.  Every frame begins INSIDE a fragment, `from` at the frame offset, no start codon seen:
//   mode 1   a fragment opens at the codon after a stop: the default rule with another stop set
//   mode 0   start codons are ignored while inside; after a stop the frame is outside, the next start codon opens a fragment there (from,
//            gap count and length begin anew), codons in between belong to nothing, and a stop or a last codon reached outside emits nothing
//   mode 2   EVERY start codon, inside or outside, sets from and resets the counts; after a stop the frame is outside until the next one
// A fragment is still emitted at its closing codon (a stop, or the frame's last complete codon), so each strand position still decides on its
// own, by a backward walk: mode 2 to the nearest start codon (a stop met first: no fragment; the frame's begin met first: incomplete start),
// mode 0 to the previous stop, remembering the FARTHEST start codon and the gap count there (none: no fragment; the frame's begin instead of a
// stop: from = frame offset, incomplete start, whatever start codons lie between).  "Incomplete start" is the reference's !hasStartCodon[frame],
// which is sticky per frame (Orf.cpp:246, 298, 344): a start event never happens before the frame's first fragment closes in mode 0, and
// in mode 2 the first fragment either begins at a start codon or at the frame offset; every later fragment needs a start event in both.  So
// the flag equals "began at the frame offset without a start codon" in all three modes.
// A codon that is a stop AND a start (no code of the table has one; the rule holds anyway): the stop decides.  The reference opens a
// fragment there in modes 0 (outside) and 2 and closes it at once with no codon (Orf.cpp:328), so in mode 2 nothing is emitted at such a codon.
__host__ __device__ __forceinline__ uint32_t plain_base(char upper) { return upper == 'A' ? 0u : upper == 'C' ? 1u : upper == 'G' ? 2u : upper == 'T' ? 3u : 4u; }

// the codon at p: bit 0 = stop, bit 1 = start, bit 2 = gap codon
template <class Tab>
__host__ __device__ __forceinline__ uint32_t codon_class(const Strand<Tab> &S, uint32_t p, const OrfRule &R) {
    const char c0 = upper_or_max(S.at(p)), c1 = upper_or_max(S.at(p + 1)), c2 = upper_or_max(S.at(p + 2));
    uint32_t cls = (not_nucleotide<Tab>(c0) || not_nucleotide<Tab>(c1) || not_nucleotide<Tab>(c2)) ? 4u : 0u;
    const uint32_t b0 = plain_base(c0), b1 = plain_base(c1), b2 = plain_base(c2);
    if ((b0 | b1 | b2) < 4u) {
        const uint32_t idx = 16u * b0 + 4u * b1 + b2;
        cls |= (uint32_t) ((R.stop_mask >> idx) & 1u) | ((uint32_t) ((R.start_mask >> idx) & 1u) << 1);
    }
    return cls;
}

// fragment_at for a rule with R.general set; MODE = R.start_mode (launch-uniform).  The walk always loads whole codons, so it always counts.
template <int MODE, class Tab>
__host__ __device__ __forceinline__ uint32_t fragment_at_modes(const Strand<Tab> &S, uint32_t p, const OrfRule &R, uint32_t &from, uint32_t &flags) {
    if (!(((S.minus ? R.reverse_frames : R.forward_frames) >> (p % 3u)) & 1u)) return 0;
    if (S.len < 3 || p + 3 > S.len) return 0;
    uint32_t cc = codon_class(S, p, R);
    const bool stop = (cc & 1u) != 0;
    const bool last = p + 6 > S.len;
    if (!stop && !last) return 0;
    if (R.end_mode < 2 && (stop ? 0u : 1u) == R.end_mode) return 0;
    uint32_t gaps = 0, q = p;                                           // gap codons of q .. p
    bool hasStart = false;
    if (MODE == 1) {
        gaps = (cc >> 2) & 1u;
        while (q >= 3) {                                                // previous stop of this frame
            cc = codon_class(S, q - 3, R);
            if (cc & 1u) { hasStart = true; break; }
            gaps += (cc >> 2) & 1u;
            if (gaps > R.max_gaps) return 0;
            q -= 3;
        }
        if (gaps > R.max_gaps) return 0;                                // (a last codon with a gap and no codon before it)
    } else if (MODE == 2) {
        if (stop && (cc & 2u)) return 0;                                // reopened and closed at once, no codon
        for (;;) {                                                      // nearest start codon at or before p
            gaps += (cc >> 2) & 1u;
            if (gaps > R.max_gaps) return 0;                            // the fragment, if there is one, holds at least these
            if (cc & 2u) { hasStart = true; break; }
            if (q < 3) break;                                           // the frame's begin: incomplete start
            q -= 3;
            cc = codon_class(S, q, R);
            if (cc & 1u) return 0;                                      // a stop and no start since: the frame is outside at p
        }
    } else {
        uint32_t startAt = 0, gapsAt = 0;
        bool begin = false;
        for (;;) {                                                      // previous stop; the farthest start codon after it wins
            gaps += (cc >> 2) & 1u;
            if ((cc & 3u) == 2u) { hasStart = true; startAt = q; gapsAt = gaps; }
            if (q < 3) { begin = true; break; }
            q -= 3;
            cc = codon_class(S, q, R);
            if (cc & 1u) break;
        }
        if (begin) hasStart = false;                                    // inside since the frame offset: the start codons were ignored
        else if (hasStart) { q = startAt; gaps = gapsAt; }
        else return 0;
        if (gaps > R.max_gaps) return 0;                                // the gaps that count are those from the farthest start
    }
    from = q;
    const uint32_t count = (p - from) / 3 + (stop ? 0u : 1u);
    if (count == 0 || count < R.min_length || count > R.max_length) return 0;
    if (R.contig_start_mode < 2 && (hasStart ? 0u : 1u) == R.contig_start_mode) return 0;      // extractorfs.cpp:84
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

// --add-orf-stop (translatenucs.cpp:57-102): flag 8 = a '*' before the first residue (complete start), flag 16 = a '*' behind the last one
// (complete end, unless the last codon already translates to '*': TAR or UAA are no stops for the scan above, and are '*' in the table)
template <class Tab>
__host__ __device__ __forceinline__ uint32_t orf_star_flags(const Strand<Tab> &S, uint32_t from, uint32_t codons, uint32_t flags, const char *table /* [4096] */) {
    uint32_t f = (flags & 1u) ? 0u : 8u;
    if (!(flags & 2u) && translate_at(S, from + 3u * (codons - 1u), table) != '*') f |= 16u;
    return f;
}
__host__ __device__ __forceinline__ uint32_t orf_star_count(uint32_t flags) { return ((flags >> 3) & 1u) + ((flags >> 4) & 1u); }

// where residue i of an n-residue fragment goes inside the fragment
__host__ __device__ __forceinline__ uint32_t orf_residue_slot(uint32_t i, uint32_t n, uint32_t reverse) { return reverse ? n - 1u - i : i; }

}  // namespace mk
