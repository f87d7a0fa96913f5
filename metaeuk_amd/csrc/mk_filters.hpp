// metaeuk_amd/csrc/mk_filters.hpp -- the result filters -c / --cov-mode / --min-seq-id, one restatement for the host paths (mk_result_filter,
// the prefilter's length cut, the host assembly) and the kernels of the alignment stage (mk_align.hip).
// Util::canBeCovered / Util::hasCoverage (M/src/commons/Util.cpp:477-511) with the reference's arithmetic: lengths converted to float, divided in
// float, compared against the float threshold; the sequence identity in double as Alignment::checkCriteria compares it (Alignment.cpp:548-550).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/metaeuk_amd.h"

namespace mk {

// Parameters.h:277-282
constexpr int COV_MODE_BIDIRECTIONAL = 0, COV_MODE_TARGET = 1, COV_MODE_QUERY = 2, COV_MODE_LENGTH_QUERY = 3, COV_MODE_LENGTH_TARGET = 4,
              COV_MODE_LENGTH_SHORTER = 5;

struct ResultFilter { float cov_thr; int cov_mode; float seq_id_thr; };
inline ResultFilter result_filter_of(const mk_params &P) { return ResultFilter{P.cov_thr, P.cov_mode, P.seq_id_thr}; }

// can the pair reach the coverage threshold at all -- a test on the two lengths (Util.cpp:477-494)
__host__ __device__ inline bool can_be_covered(float covThr, int covMode, float queryLength, float targetLength) {
    switch (covMode) {
        case COV_MODE_BIDIRECTIONAL: return (queryLength / targetLength >= covThr) && (targetLength / queryLength >= covThr);
        case COV_MODE_QUERY: return (targetLength / queryLength) >= covThr;
        case COV_MODE_TARGET: return (queryLength / targetLength) >= covThr;
        case COV_MODE_LENGTH_QUERY: return ((targetLength / queryLength) >= covThr) && (targetLength / queryLength) <= 1.0f;
        case COV_MODE_LENGTH_TARGET: return ((queryLength / targetLength) >= covThr) && (queryLength / targetLength) <= 1.0f;
        case COV_MODE_LENGTH_SHORTER: {
            const float lo = targetLength < queryLength ? targetLength : queryLength, hi = targetLength < queryLength ? queryLength : targetLength;
            return (lo / hi) >= covThr;
        }
        default: return true;
    }
}

// Util.cpp:496-511: the length modes 3 to 5 always pass
__host__ __device__ inline bool has_coverage(float covThr, int covMode, float queryCov, float targetCov) {
    switch (covMode) {
        case COV_MODE_BIDIRECTIONAL: return (queryCov >= covThr) && (targetCov >= covThr);
        case COV_MODE_QUERY: return queryCov >= covThr;
        case COV_MODE_TARGET: return targetCov >= covThr;
        default: return true;
    }
}

__host__ __device__ inline bool seq_id_ok(float seqId, float seqIdThr) { return (double) seqId >= (double) seqIdThr; }

// The alignment stage takes its filter path (length cut, coverage gate) only when a filter can drop something: a threshold above 0 -- or the
// `<= 1.0` clause of the length modes 3 and 4, which the reference applies at -c 0 as well (Alignment.cpp:370).
__host__ __device__ inline bool filters_active(const ResultFilter &F) {
    return F.cov_thr > 0.0f || F.seq_id_thr > 0.0f || F.cov_mode == COV_MODE_LENGTH_QUERY || F.cov_mode == COV_MODE_LENGTH_TARGET;
}
// the prefilter's cut (Prefiltering.cpp:856-863)
inline bool prefilter_cut_active(const ResultFilter &F) {
    return F.cov_thr > 0.0f && (F.cov_mode == COV_MODE_BIDIRECTIONAL || F.cov_mode == COV_MODE_QUERY || F.cov_mode == COV_MODE_LENGTH_SHORTER);
}
inline bool filter_in_range(const ResultFilter &F) {
    return F.cov_mode >= 0 && F.cov_mode <= 5 && F.cov_thr >= 0.0f && F.cov_thr <= 1.0f && F.seq_id_thr >= 0.0f && F.seq_id_thr <= 1.0f;
}

}  // namespace mk
