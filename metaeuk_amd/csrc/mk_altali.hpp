// metaeuk_amd/csrc/mk_altali.hpp -- alternative alignments (`align` / `search --alt-ali N`), one restatement for the host twin
// (mk_alt_alignments_host) and the kernel of mk_altali.hip.  M/src/alignment/Alignment.cpp:399-401, 569-601 (computeAlternativeAlignment).
// Kept from the reference:
//  - only the records the ordinary stage accepted are origins (firstItResSize); an alternative never starts a chain of its own;
//  - the mask of a chain is the origin's [db_start, db_end) plus [db_start, db_end) of every alternative the chain accepted so far.  The loop is
//    `pos < dbEndPos`: the LAST aligned target residue stays unmasked, and an interval with db_start == db_end masks nothing -- the chain then
//    finds the same alignment again, up to N times.  Reproduced, not repaired;
//  - every origin starts from the unmasked target (mapSequence again): the masks of other origins on the same target do not apply;
//  - a masked residue is code 20 (X), scored through the query's matrix + composition-bias profile like any residue;
//  - a round is a full getSWResult in SCORE_COV mode: forward score; end cell = first column of the maximum, smallest row in it; the e-value
//    with the query length and the database size unchanged; the early return on the e-value and on the coverage over (0, end cell)
//    (StripedSmithWaterman.cpp:389-398); the reverse pass for the start; the record (Matcher.cpp:100-164); Alignment::checkCriteria;
//  - a rejected round ends the chain.
// Defined here where the reference is not: Matcher::compareHits ends at the DB key, so two records of one target can tie completely and the
// reference's std::sort leaves their order open; here ties keep chain order (origin, then its alternatives by round).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../include/metaeuk_amd.h"
#include "mk_filters.hpp"

namespace mk {

constexpr int ALTALI_MAX = 32;                    // largest --alt-ali: a chain's ALTALI_MAX + 1 intervals sit in LDS beside the query profile
// the kernel's work split (mk_altali.hip): rows per lane; queries of at most ALTALI_SMALL_ROWS rows run on 8-lane groups, eight chains per wave,
// longer ones on the whole wave in row tiles of ALTALI_TILE_ROWS; a lane loads one aligned dword of the target per block, so a block is
// 4 x (lanes of the group) columns
constexpr int ALTALI_R = 8, ALTALI_SMALL_ROWS = 8 * ALTALI_R, ALTALI_TILE_ROWS = 64 * ALTALI_R;
constexpr int ALTALI_SMALL_BLOCK = 4 * 8, ALTALI_LARGE_BLOCK = 4 * 64;
constexpr uint32_t ALTALI_X = 20;                 // the code a masked residue is replaced with

struct AltInterval { int32_t start, end; };       // [start, end) of the target
__host__ __device__ inline bool altali_masked(const AltInterval *iv, int n, int pos) {
    bool m = false;
    for (int k = 0; k < n; k++) m |= pos >= iv[k].start && pos < iv[k].end;
    return m;
}
// score of a cell: the int8 profile entry of ssw_init (matrix + composition bias, stored as int8)
__host__ __device__ inline int altali_cell(const int8_t *mat, uint32_t qRes, int bias, uint32_t tRes) {
    return (int) (int8_t) ((int) mat[(tRes < 20u ? tRes : 20u) * 21u + (qRes < 20u ? qRes : 20u)] + bias);
}

struct AltCriteria { double evalThr; int minAlnLen; ResultFilter filter; int gapOpen, gapExtend; };
inline AltCriteria altali_criteria_of(const mk_params &P) { return AltCriteria{P.evalue_thr, P.min_aln_len, result_filter_of(P), P.gap_open, P.gap_extend}; }

__host__ __device__ inline float altali_cov(unsigned s, unsigned e, unsigned len) {      // SmithWaterman::computeCov
    const unsigned hi = s > e ? s : e, lo = s < e ? s : e;
    return (float) ((len < hi ? len : hi) - lo + 1u) / (float) len;
}
// ssw_align_private's early return (StripedSmithWaterman.cpp:389-398): false = no reverse pass, the round is rejected
__host__ __device__ inline bool altali_gate(const AltCriteria &C, double evalue, int qEnd, int tEnd, int qLen, int tLen) {
    if (evalue > C.evalThr) return false;
    return has_coverage(C.filter.cov_thr, C.filter.cov_mode, altali_cov(0u, (unsigned) qEnd, (unsigned) qLen), altali_cov(0u, (unsigned) tEnd, (unsigned) tLen));
}
// Matcher::getSWResult's tail (Matcher.cpp:100-164) and Alignment::checkCriteria (Alignment.cpp:548-567) for one round behind the gate
__host__ __device__ inline bool altali_record(const AltCriteria &C, uint32_t target, int score, int qStart, int qEnd, int tStart, int tEnd, int qLen, int tLen,
                                              double evalue, int bitScore, mk_alignment &a) {
    a.db_key = target; a.q_len = qLen; a.db_len = tLen; a.raw_score = score; a.evalue = evalue; a.bit_score = bitScore;
    a.qcov = altali_cov((unsigned) qStart, (unsigned) qEnd, (unsigned) qLen);
    a.dbcov = altali_cov((unsigned) tStart, (unsigned) tEnd, (unsigned) tLen);
    a.q_start = qStart; a.q_end = qEnd; a.db_start = tStart; a.db_end = tEnd;
    const int dq = qEnd - qStart, dt = tEnd - tStart;
    a.aln_len = ((dq < 0 ? -dq : dq) > (dt < 0 ? -dt : dt) ? (dq < 0 ? -dq : dq) : (dt < 0 ? -dt : dt)) + 1;
    const unsigned qAln = (unsigned) qEnd - (unsigned) qStart > 1u ? (unsigned) qEnd - (unsigned) qStart : 1u;
    const unsigned dbAln = (unsigned) tEnd - (unsigned) tStart > 1u ? (unsigned) tEnd - (unsigned) tStart : 1u;
    const uint16_t s16 = (uint16_t) score;
    float sid = (float) ((double) ((float) (int) s16 / (float) (qAln > dbAln ? qAln : dbAln)) * 0.1656 + 0.1141);   // Matcher.cpp:160-164 (float / float, then double)
    sid = fminf(sid, 1.0f);
    a.seq_id = fmaxf(0.0f, sid);
    return a.evalue <= C.evalThr && a.aln_len >= C.minAlnLen && has_coverage(C.filter.cov_thr, C.filter.cov_mode, a.qcov, a.dbcov) &&
           seq_id_ok(a.seq_id, C.filter.seq_id_thr);
}

// plain Gotoh over rows x cols cells, int32, saturating at 32 767 like the kernels (mk_sw.hip): the maximum, the first column that reaches it and the
// smallest row there.  score_of(row, col) = altali_cell of the pass's row and column.  The host twin's pass.
struct AltSw { int score = 0, end_row = -1, end_col = -1; };
template <class ScoreFn>
inline AltSw altali_gotoh(ScoreFn score_of, int rows, int cols, int gapOpen, int gapExtend) {
    std::vector<int> H((size_t) rows, 0), E((size_t) rows, 0);
    AltSw best;
    for (int c = 0; c < cols; c++) {
        int diag = 0, F = 0;
        for (int r = 0; r < rows; r++) {
            const int sc = score_of(r, c);
            const int d = diag + sc < 32767 ? diag + sc : 32767;
            diag = H[(size_t) r];
            int h = d > E[(size_t) r] ? d : E[(size_t) r];
            h = h > F ? h : F;
            if (h > best.score) { best.score = h; best.end_row = r; best.end_col = c; }
            const int ho = h - gapOpen;
            E[(size_t) r] = E[(size_t) r] - gapExtend > ho ? E[(size_t) r] - gapExtend : ho;
            if (E[(size_t) r] < 0) E[(size_t) r] = 0;
            F = F - gapExtend > ho ? F - gapExtend : ho;
            if (F < 0) F = 0;
            H[(size_t) r] = h;
        }
    }
    return best;
}

// ---- the kernel side (mk_altali.hip) ----
// A chain = one origin; a job of a round = an open chain.  Everything below is device memory.
struct AltView {
    const uint8_t *q_res; const int8_t *q_bias8; const uint64_t *q_off;
    const uint8_t *t_res; const uint64_t *t_off; const int8_t *mat;         // mat: 21 x 21 int8
    const uint32_t *chain_q, *chain_t;            // per chain: query and target
    uint32_t *chain_niv; AltInterval *chain_iv;   // per chain: intervals so far, [chain][alt_ali + 1]; an accepted round appends its own
    uint32_t iv_stride;                           // alt_ali + 1
    const uint32_t *jobs; uint32_t n_jobs;        // the round's open chains
    const double *evalTab; const int32_t *lenIdx; uint32_t maxLen, smax; const int32_t *bitScore;
    AltCriteria crit;
    mk_alignment *rec; uint8_t *verdict;          // per job: the record; ALT_REJECTED / ALT_ACCEPTED / ALT_BEYOND_TABLE
    uint32_t *border; uint32_t border_stride, border_slots;   // row tiles: per slot one packed (H | F << 16) per column; *border_next hands out slots
    uint32_t *border_next;
    uint32_t *flags;                              // [0] forward / reverse mismatch, [1] no border slot left
    unsigned long long *work;                     // [0] algorithmic bytes, [1] cells
};
constexpr uint8_t ALT_REJECTED = 0, ALT_ACCEPTED = 1, ALT_BEYOND_TABLE = 2;
hipError_t launch_altali(const AltView &V, bool anyLarge, hipStream_t stream);
// the next round's job list: the accepted jobs in their order (count, scan, emit).  blockCnt: device scratch, one word per 256 jobs + 1;
// *total (device) = their number
hipError_t launch_altali_compact(const uint32_t *jobs, const uint8_t *verdict, uint32_t n, uint32_t *blockCnt, uint32_t *nextJobs, uint32_t *total, hipStream_t stream);

}  // namespace mk
