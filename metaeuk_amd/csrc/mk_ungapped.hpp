// metaeuk_amd/csrc/mk_ungapped.hpp -- the exhaustive gapless prefilter (`ungappedprefilter`, `search --prefilter-mode 1`), one restatement for the
// host twin (mk_ungapped_prefilter_host) and the kernels of mk_ungapped.hip.  M/src/prefiltering/ungappedprefilter.cpp:338-477 (runFilterOnCpu
// with alignmentMode == 0) and SmithWaterman::ungapped_alignment, M/src/alignment/StripedSmithWaterman.cpp:1722-1781.
// Kept from the reference:
//  - ssw_init (:1276-1287): bias = |min(0, the 441 matrix entries)| + |min(0, the query's int8 composition bias)|, a constant of the query; the byte
//    profile holds (int8) (mat[t][q_i] + comp_bias[i] + bias), read back as an unsigned byte (createQueryProfile, :174).
//  - the recurrence in unsigned bytes: S(i, j) = subs_u8(adds_u8(S(i-1, j-1), profile byte), bias), S = 0 outside the rectangle, the pair's score the
//    maximum over all cells.  The striped layout is only a layout: the byte shift at a stripe head hands row b W - 1 to row b W, and the padded rows
//    behind the query carry the byte `bias`, change nothing and feed only padded rows -- the score does not depend on the SIMD width.
//  - per pair (:403-452): skipped when Util::canBeCovered fails, kept when score > --min-ungapped-score (strictly); per query (:462-467) the hits
//    sorted with hit_t::compareHitsByScoreAndId (score descending, DB key ascending) and the first --max-seqs kept.
// The commuted form the kernel uses: with b = the profile byte, the two saturating steps are S' = max(0, min(S + b, 255) - bias)
// = max(0, min(S + (b - bias), 255 - bias)).  A capped and an uncapped run agree until the first cell that reaches 255 - bias; from there the capped
// maximum is 255 - bias and the uncapped one at least that.  So score = min(255 - bias, max over cells of U), U(i, j) = max(0, U(i-1, j-1) + (b - bias))
// in anything wide enough (saturating int16 here: a U that sticks at 32767 has long passed the cap).
// Profile queries (the inverted search of a profile target database: ungappedprefilter.cpp:373-374 hands qSeq.getAlignmentProfile() to ssw_init).
// The byte of column i and residue a is P[i][a] + bias with P the int8 alignment profile (the 20 amino-acid entries of the [column][32] array of
// mk_profile.hpp), X (code 20, and any code above it) scores 0 in every column (ssw_init clears that row, StripedSmithWaterman.cpp:1243-1244),
// bias = |min(0, the 20 amino-acid scores of all columns)| (:1276-1287 with matSize = L * PROFILE_AA_SIZE), and a profile has no composition bias.
// The recurrence, the commuted form, the verdicts, the order and the cut are the ones above: ungapped_profile_* below and the same helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include "../../include/metaeuk_amd.h"
#include "mk_filters.hpp"

namespace mk {

constexpr int PREF_MODE_KMER = 0, PREF_MODE_UNGAPPED = 1, PREF_MODE_EXHAUSTIVE = 2, PREF_MODE_UNGAPPED_AND_GAPPED = 3;    // Parameters.h: PREF_MODE_*

// the kernel's work split (mk_ungapped.hip): diagonals per lane, queries per packed lookup, rows of the profile image in LDS, lanes per target for
// short and for long targets, the target length from which a whole wave sweeps one target, the budget of the score array
constexpr int UNG_DIAGS = 8, UNG_PACK = 4, UNG_ROW_TILE = 128, UNG_GROUP_SHORT = 8, UNG_GROUP_LONG = 64, UNG_LONG_TARGET = 2048;
constexpr uint64_t UNG_SCORE_BUDGET = 256ull << 20;
constexpr int UNG_PAD_CODE = 31;                      // the residue code of a window position outside the target: its image line clears the state

// ssw_init's bias; matMin = the minimum of the 441 matrix entries and 0, biasMin = the minimum of the query's composition bias and 0
__host__ __device__ inline int ungapped_bias(int matMin, int biasMin) { return (matMin < 0 ? -matMin : matMin) + (biasMin < 0 ? -biasMin : biasMin); }
// the profile byte of one cell (createQueryProfile: the int8 store, read unsigned)
__host__ __device__ inline uint8_t ungapped_profile_byte(int matScore, int compBias, int bias) { return (uint8_t) (matScore + compBias + bias); }
// the literal byte step: adds_u8, then subs_u8
__host__ __device__ inline uint8_t ungapped_step(uint8_t s, uint8_t profileByte, uint8_t bias) {
    const unsigned a = (unsigned) s + (unsigned) profileByte;
    const unsigned sat = a > 255u ? 255u : a;
    return (uint8_t) (sat > (unsigned) bias ? sat - (unsigned) bias : 0u);
}
// what the commuted form adds per cell, and its cap
__host__ __device__ inline int ungapped_cell(int matScore, int compBias, int bias) { return (int) ungapped_profile_byte(matScore, compBias, bias) - bias; }
__host__ __device__ inline int ungapped_cap(int bias) { return 255 - bias; }

// the pair's verdict in front of the score (Util::canBeCovered) and behind it (hasDiagScore)
__host__ __device__ inline bool ungapped_pair_scored(float covThr, int covMode, uint32_t qLen, uint32_t tLen) {
    return can_be_covered(covThr, covMode, (float) qLen, (float) tLen);
}
__host__ __device__ inline bool ungapped_hit_kept(int score, int minUngappedScore) { return score > minUngappedScore; }

// hit_t::compareHitsByScoreAndId as one ascending key: (255 - score) above the DB key (or its rank among the database's keys: the same order)
__host__ __device__ inline uint64_t ungapped_hit_key(uint32_t score, uint32_t key) { return ((uint64_t) (255u - score) << 32) | key; }
__host__ __device__ inline bool ungapped_hit_before(uint32_t scoreA, uint32_t keyA, uint32_t scoreB, uint32_t keyB) {
    return ungapped_hit_key(scoreA, keyA) < ungapped_hit_key(scoreB, keyB);
}

// one pair, cell by cell, in the literal byte arithmetic (the twin).  mat = 21 x 21 int8, bias8 = the query's composition bias or nullptr
inline int ungapped_pair_host(const int8_t *mat, const uint8_t *q, const int8_t *bias8, int qLen, const uint8_t *t, int tLen) {
    int matMin = 0, biasMin = 0;
    for (int i = 0; i < 441; i++) matMin = mat[i] < matMin ? mat[i] : matMin;
    for (int i = 0; bias8 && i < qLen; i++) biasMin = bias8[i] < biasMin ? bias8[i] : biasMin;
    const int bias = ungapped_bias(matMin, biasMin);
    uint8_t best = 0;
    for (int d = -(qLen - 1); d < tLen; d++) {          // diagonal d: row i meets column d + i
        uint8_t s = 0;
        for (int i = d < 0 ? -d : 0; i < qLen && d + i < tLen; i++) {
            const int qc = q[i] < 20 ? q[i] : 20, tc = t[d + i] < 20 ? t[d + i] : 20;
            s = ungapped_step(s, ungapped_profile_byte(mat[tc * 21 + qc], bias8 ? bias8[i] : 0, bias), (uint8_t) bias);
            best = s > best ? s : best;
        }
    }
    return best;
}

// ---- profile queries ----
// the work split of ungapped_profile_scores_kernel: lanes per target (a band is UNG_PROF_GROUP * UNG_DIAGS diagonals), target positions per
// image window, the largest number of targets a lane group takes per band
constexpr int UNG_PROF_GROUP = 16, UNG_PROF_BAND = UNG_PROF_GROUP * UNG_DIAGS, UNG_PROF_TILE = 128, UNG_PROF_MAX_PASSES = 16;
// what column `col` ([32] int8, mk_profile.hpp) scores for residue code `code`
__host__ __device__ inline int ungapped_profile_score(const int8_t *col, int code) { return code < 20 ? (int) col[code] : 0; }
// the smallest amino-acid score of a column and 0
__host__ __device__ inline int ungapped_profile_col_min(const int8_t *col) {
    int m = 0;
    for (int a = 0; a < 20; a++) m = col[a] < m ? col[a] : m;
    return m;
}
// one pair, cell by cell, in the literal byte arithmetic (the twin).  aln32 = [nCols][32] int8
inline int ungapped_profile_pair_host(const int8_t *aln32, int nCols, const uint8_t *t, int tLen) {
    int pMin = 0;
    for (int i = 0; i < nCols; i++) { const int m = ungapped_profile_col_min(aln32 + (size_t) i * 32); pMin = m < pMin ? m : pMin; }
    const int bias = ungapped_bias(pMin, 0);
    uint8_t best = 0;
    for (int e = -(tLen - 1); e < nCols; e++) {         // diagonal e: target position j meets column e + j
        uint8_t s = 0;
        for (int j = e < 0 ? -e : 0; j < tLen && e + j < nCols; j++) {
            s = ungapped_step(s, ungapped_profile_byte(ungapped_profile_score(aln32 + (size_t) (e + j) * 32, t[j]), 0, bias), (uint8_t) bias);
            best = s > best ? s : best;
        }
    }
    return best;
}

// ---- the kernel side (mk_ungapped.hip) ----
struct UngappedView {
    const uint8_t *q_res; const uint64_t *q_off; const int8_t *q_bias8; uint32_t n_queries;
    const uint32_t *q_order;                   // the batch's queries by ascending length; four neighbours share a lookup
    const uint8_t *q_cap;                      // [query] 255 - bias (ungapped_caps)
    const uint8_t *t_res; const uint64_t *t_off; uint32_t n_targets;
    const uint32_t *t_order;                   // the targets by ascending length
    const int8_t *mat;                         // 21 x 21 int8 [t * 21 + q]
    int mat_min;
    float cov_thr; int cov_mode;
    uint32_t q0, nq;                           // the chunk's queries: positions [q0, q0 + nq) of q_order, q0 a multiple of UNG_PACK
    uint32_t s0, ns;                           // the chunk's targets: positions [s0, s0 + ns) of t_order
    uint8_t *scores;                           // [nq][ns] one byte per pair, 0 for a skipped pair
    unsigned long long *work;                  // [0] algorithmic bytes, [1] cells
    const int8_t *p_aln = nullptr;             // profile queries: [column][32] alignment profile, q_off the column offsets (q_res, q_bias8, mat unused)
};
// 255 - bias of every query
hipError_t launch_ungapped_caps(const UngappedView &V, uint8_t *caps, hipStream_t stream);
// the same for every profile of a profile batch (V.p_aln)
hipError_t launch_ungapped_profile_caps(const UngappedView &V, uint8_t *caps, hipStream_t stream);
// profile queries: the scores of positions [a, b) of the chunk's targets, every lane group taking `passes` targets per band of diagonals
// (1 .. UNG_PROF_MAX_PASSES; 1 when a target of the range is longer than UNG_PROF_TILE)
hipError_t launch_ungapped_profile_scores(const UngappedView &V, uint32_t a, uint32_t b, uint32_t passes, hipStream_t stream);
// the scores of positions [a, b) of the chunk's targets with `group` lanes per target (UNG_GROUP_SHORT or UNG_GROUP_LONG)
hipError_t launch_ungapped_scores(const UngappedView &V, uint32_t a, uint32_t b, int group, hipStream_t stream);
// the best max_seqs hits of every query of the chunk over the chunk's targets and the candidates kept from earlier target chunks (cand / cand_cnt, in
// and out: [nq][max_seqs] keys of ungapped_hit_key over the key RANK, ascending).  key_rank / rank_idx: the rank of a target's DB key among all
// keys and its inverse (nullptr: key = index).  last: writes hits[nq][max_seqs] and hit_cnt[nq] as well
struct UngappedSelect {
    const uint32_t *key_rank, *rank_idx; int min_score; uint32_t max_seqs;
    uint64_t *cand; uint32_t *cand_cnt; uint64_t *tmp;      // tmp: [nq][max_seqs] scratch of one round
    mk_hit *hits; uint32_t *hit_cnt; bool last;
};
hipError_t launch_ungapped_select(const UngappedView &V, const UngappedSelect &S, hipStream_t stream);

}  // namespace mk
