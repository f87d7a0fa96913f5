// metaeuk_amd/csrc/mk_rescore.hpp -- the ungapped rescoring of prefilter hits (`rescorediagonal --rescore-mode 2`, RESCORE_MODE_ALIGNMENT, the
// mode `search --alignment-mode 4` selects, Search.cpp:387), one restatement for the host twin (mk_rescore_diagonal_host) and the kernel of
// mk_rescore.hip.  M/src/alignment/DistanceCalculator.h:93-201 and M/src/alignment/rescorediagonal.cpp:193-342.
// Kept from the reference:
//  - computeUngappedAlignment (:93-113) ALWAYS walks the real diagonals a 16-bit value can stand for: -d * 65536 + diagonal for
//    d = 1 .. 1 + tLen / 32768, then d * 65536 + diagonal for d = 0 .. qLen / 65536 (unsigned wrap, then int), and a later one replaces the
//    best only when its score is strictly greater.  For sequences below 32768 that is the signed value and one more that misses the rectangle.
//  - ungappedAlignmentByDiagonal (:115-175): diagonal >= 0 goes |diagonal| into the query, < 0 into the target; a real diagonal that does not
//    cross the rectangle scores 0 (and so never replaces anything).
//  - computeSubstitutionStartEndDistance (:178-201): running sum clamped at 0, a reset at `score <= 0` sets minPos = pos, a new maximum only on
//    strictly greater: the end is the FIRST position of the maximum, the start one behind the LAST reset before it, no positive cell gives 0 / 0 / 0.
//  - the scores are the alignment stage's matrix (SubstitutionMatrix 2.0, 0.0) on the unmasked residues, summed in int: no composition bias, no
//    saturation (this is not mk_kernels.hpp: ungapped_score).
//  - the record (rescorediagonal.cpp:239-307) and the verdict (:211, :314-322) with the reference's float / double expression types.
// The prefix-sum form the kernel uses gives the same answers: P[i] = plain prefix sum, P[-1] = 0, s[i] = P[i] - min(P[-1 .. i]); the end is the first
// argmax of s, the start (last argmin of P[-1 .. end]) + 1; RescoreState::step is that form, cell by cell, and a lane may start it from any carried
// (sum, min, min position).
// Defined here where the reference is not: when NO real diagonal has a positive score the reference keeps its empty LocalAlignment (start = end =
// -1, diagonal 0) and then counts identities on the bytes in front of both sequences; here such a pair has 0 identities.  Its record (aln_len 1,
// coordinates -1) is otherwise the reference's.  A 16-bit diagonal none of whose real diagonals crosses the rectangle is an argument error.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/metaeuk_amd.h"
#include "mk_align.hpp"
#include "mk_filters.hpp"
#include "mk_trace.hpp"

namespace mk {

constexpr int RESCORE_MODE_ALIGNMENT = 2;               // Parameters.h: RESCORE_MODE_ALIGNMENT
// the kernel's work split (mk_rescore.hip): lanes per pair, cells per lane and sweep
constexpr int RESCORE_GROUP = 8, RESCORE_SEG = 8, RESCORE_SWEEP = RESCORE_GROUP * RESCORE_SEG;

// the walk of one diagonal in prefix-sum form.  sum = P[i]; (minVal, minPos) = the LATEST minimum of P[-1 .. i]; best = max of s so far with the
// positions of its FIRST occurrence
struct RescoreState {
    int32_t sum = 0, minVal = 0, minPos = -1, best = 0, bestStart = 0, bestEnd = 0;
    __host__ __device__ inline void step(int32_t curr, int32_t pos) {
        sum += curr;
        if (sum <= minVal) { minVal = sum; minPos = pos; }          // score <= 0: reset, minPos = pos (equal minima: the latest)
        const int32_t s = sum - minVal;
        if (s > best) { best = s; bestEnd = pos; bestStart = minPos + 1; }   // strictly greater: the first position of the maximum
    }
};

// the part of the rectangle a real diagonal crosses (ungappedAlignmentByDiagonal, :119-125, :148-150); len = 0: it misses the rectangle
struct RescoreDiag { uint32_t q0, t0, len; };
__host__ __device__ inline RescoreDiag rescore_geometry(int real, uint32_t qLen, uint32_t tLen) {
    const uint32_t dist = (uint32_t) (real < 0 ? -(int64_t) real : (int64_t) real);
    RescoreDiag g{0, 0, 0};
    if (real >= 0 && dist < qLen) { g.q0 = dist; g.len = tLen < qLen - dist ? tLen : qLen - dist; }
    else if (real < 0 && dist < tLen) { g.t0 = dist; g.len = tLen - dist < qLen ? tLen - dist : qLen; }
    return g;
}
// the real diagonals of a 16-bit one in the reference's order (computeUngappedAlignment, :98-111)
__host__ __device__ inline uint32_t rescore_candidates(uint32_t qLen, uint32_t tLen) { return (1u + tLen / 32768u) + (qLen / 65536u + 1u); }
__host__ __device__ inline int rescore_candidate(uint32_t k, uint32_t d16, uint32_t tLen) {
    const uint32_t nNeg = 1u + tLen / 32768u;
    return k < nNeg ? (int) (0u - (k + 1u) * 65536u + d16) : (int) ((k - nNeg) * 65536u + d16);
}
__host__ __device__ inline bool rescore_diagonal_valid(uint32_t d16, uint32_t qLen, uint32_t tLen) {
    for (uint32_t k = 0; k < rescore_candidates(qLen, tLen); k++) if (rescore_geometry(rescore_candidate(k, d16, tLen), qLen, tLen).len) return true;
    return false;
}

// the best real diagonal of a pair: the reference's LocalAlignment after computeUngappedAlignment.  found = false: the empty one
struct RescoreBest { int32_t score = 0, start = -1, end = -1, real = 0; bool found = false; };
__host__ __device__ inline void rescore_offer(RescoreBest &b, const RescoreState &s, int real) {
    if (s.best > b.score) { b.score = s.best; b.start = s.bestStart; b.end = s.bestEnd; b.real = real; b.found = true; }
}

// SmithWaterman::computeCov (StripedSmithWaterman.h), unsigned as the reference declares it
__host__ __device__ inline float rescore_cov(unsigned s, unsigned e, unsigned len) {
    const unsigned hi = s > e ? s : e, lo = s < e ? s : e;
    return (float) ((len < hi ? len : hi) - lo + 1u) / (float) len;
}

struct RescoreCriteria { double evalThr; int minAlnLen; ResultFilter filter; int seqIdMode; };
inline RescoreCriteria rescore_criteria_of(const mk_params &P) { return RescoreCriteria{P.evalue_thr, P.min_aln_len, result_filter_of(P), P.seq_id_mode}; }

// rescorediagonal.cpp:239-322 for one pair behind Util::canBeCovered: the record and the verdict hasAlnLen && hasCov && hasSeqId && hasEvalue.
// identities = equal residues over [start, end] (0 for the empty alignment); evalue / bitScore = computeEvalue(score, qLen) and
// (int) (computeBitScore(score) + 0.5) from the host's tables.  The sequence identity is only computed when the e-value passes (:284); seqId is a
// double there, the threshold a float minus the float epsilon (:316).
__host__ __device__ inline bool rescore_record(const RescoreCriteria &C, const RescoreBest &b, uint32_t target, int qLen, int tLen, int identities,
                                               double evalue, int bitScore, mk_alignment &a) {
    const int alnLen = b.end - b.start + 1;
    const int dist = b.real < 0 ? -b.real : b.real;
    a.db_key = target; a.bit_score = bitScore; a.evalue = evalue; a.q_len = qLen; a.db_len = tLen; a.aln_len = alnLen; a.raw_score = b.score;
    if (b.real >= 0) { a.q_start = b.start + dist; a.q_end = b.end + dist; a.db_start = b.start; a.db_end = b.end; }
    else { a.q_start = b.start; a.q_end = b.end; a.db_start = b.start + dist; a.db_end = b.end + dist; }
    double seqId = 0;
    if (evalue <= C.evalThr) seqId = compute_seq_id(C.seqIdMode, identities, qLen, tLen, alnLen);
    a.seq_id = (float) seqId;
    a.qcov = rescore_cov((unsigned) a.q_start, (unsigned) a.q_end, (unsigned) qLen);
    a.dbcov = rescore_cov((unsigned) a.db_start, (unsigned) a.db_end, (unsigned) tLen);
    const bool hasCov = has_coverage(C.filter.cov_thr, C.filter.cov_mode, a.qcov, a.dbcov);
    const bool hasSeqId = seqId >= (double) (float) (C.filter.seq_id_thr - 1.1920928955078125e-07f);
    return alnLen >= C.minAlnLen && hasCov && hasSeqId && evalue <= C.evalThr;
}

// ---- the kernel side (mk_rescore.hip) ----
struct RescoreView {
    const uint8_t *q_res; const uint64_t *q_off; uint32_t n_queries;
    const uint8_t *t_res; const uint64_t *t_off; uint32_t n_targets;
    const int8_t *mat;                         // 21 x 21 int8 [q * 21 + t]
    const uint64_t *hit_off; const mk_hit *hits; uint64_t n_pairs;      // the prefilter lists, on the device
    const double *evalTab; const int32_t *lenIdx; uint32_t maxLen, smax; const int32_t *bitScore;
    RescoreCriteria crit;
    AlnRaw *raw; mk_alignment *rec; uint8_t *pass;    // per pair of the list (raw: only .pair, for the shared order kernels)
    uint32_t *flags;                           // [0] score beyond the e-value table, [1] a diagonal that misses the rectangle / a target out of range
    unsigned long long *work;                  // [0] algorithmic bytes, [1] cells
};
hipError_t launch_rescore(const RescoreView &V, hipStream_t stream);
// the accepted records of every query in output order: list order (sorted = false) or Matcher::compareHits (the alignment stage's rank kernel).
// cnt / off: device [n_queries] / [n_queries + 1] (off[n_queries] = the total); out: device, room for n_pairs records.  mk_align.hip
int rescore_order_device(const RescoreView &V, bool sorted, const uint32_t *sortKey, uint32_t *cnt, uint32_t *off, mk_alignment *out, hipStream_t stream,
                         std::string &err);

}  // namespace mk
