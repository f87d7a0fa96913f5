// metaeuk_amd/csrc/mk_gapped.hpp -- the exhaustive gapped prefilter (`gappedprefilter`), one restatement for the host twin
// (mk_gapped_prefilter_host) and the kernels of mk_gapped.hip.  M/src/prefiltering/ungappedprefilter.cpp:338-477 (runFilterOnCpu with
// alignmentMode != 0) and SmithWaterman::ssw_align with Matcher::SCORE_ONLY, M/src/alignment/StripedSmithWaterman.cpp:278-373.
// Kept from the reference:
//  - the score: score1 of ssw_align, the byte pass and, when that returns 255, the word pass.  Cell by cell both are plain local Gotoh (DESIGN.md 2,
//    "SW recurrence and why the SIMD width cannot leak"): H(i, j) = max(0, H(i-1, j-1) + s(i, j), E(i, j), F(i, j)), E(i, j+1) = max(E(i, j) - ge,
//    H(i, j) - go), F(i+1, j) = max(F(i, j) - ge, H(i, j) - go), s = matrix entry + the query row's int8 composition bias, go = 11, ge = 1, the
//    score the maximum over all cells, the additions saturating at 32 767 (the word pass's adds_epi16): a score is capped there.
//  - per pair (:403-452): skipped when Util::canBeCovered fails; kept when score > --min-ungapped-score (strictly) and, with an e-value threshold
//    below DBL_MAX, computeEvalue(score, qLen) <= threshold with the GAPPED parameter set (the evaluer is built with the gap costs, :537);
//    per query (:462-467) the hits sorted with hit_t::compareHitsByScoreAndId (score descending, DB key ascending), the first --max-seqs kept.
// The form both sides use keeps E and F at 0 and above (the reference's subs_epu16 on the gap costs): with E^ = max(E, 0), F^ = max(F, 0) the cell
// H = max(H(i-1, j-1) + s, E^, F^) is the same H (a negative E or F never wins against the 0), and E^' = max(E^ - ge, H - go, 0) = max(E', 0).
// THE PADDING ARGUMENT.  The kernel walks tiles of G x R rows and packs two queries of different length in the halves of a register, so it walks rows
// behind a query's end; and a lane group walks G - 1 columns in front of and behind its target.  Such a row or column adds GAP_PAD = -32768: the
// diagonal term H(i-1, j-1) + s is then negative, and the cell is max(E^, F^).  In a pad ROW E starts at 0 and F comes down from the real cell above
// it in the same column, F = max(F_above - ge, H_above - go) < H_above (go, ge >= 1): by induction over the pad rows and along them every pad cell
// is 0 or strictly below a real cell of the pair.  In a pad COLUMN behind the target the same holds with E coming from the real cell to the left; in
// front of the target everything is 0.  A pad cell never raises the pair's maximum, and no real cell reads one: pad rows lie below, pad columns
// outside.  (A pad row's H is also handed on as the diagonal term of the next pad row, where -32768 clears it again.)
// Profile queries (the inverted search of a profile target database: ungappedprefilter.cpp:373-374 hands qSeq.getAlignmentProfile() to ssw_init,
// StripedSmithWaterman.cpp:1228-1247): column i and residue a score P[i][a], the int8 alignment profile (entries 0..19 of the [column][32] array of
// mk_profile.hpp); X and every code above it score 0 in every column; there is no composition bias; GAP_POS_SCORING is not defined, so the gap costs
// are the uniform 11 / 1.  Cell, running maximum, cap, verdicts, order and cut are the ones above with the column count as the query length.
// THE PADDING ARGUMENT, TRANSPOSED.  gapped_profile_scores_kernel puts the TARGET in the rows (8 lanes x R residues) and walks the profile's columns
// in blocks of four, lane l one block behind lane l - 1.  Pad ROWS now lie behind a target's end (a target shorter than 8 R); pad COLUMNS lie in
// front of column 0 (the lane lag: 7 blocks), behind the end of the shorter profile of a register pair, and behind the longer one's end (the
// ramp-out and the rest of its last block).  gapped_cell is symmetric in E and F: exchanging rows and columns exchanges the two and nothing else, so
// the argument above holds with the roles swapped, and written out it reads: a pad cell adds GAP_PAD, so it is max(E^, F^).  In a pad column in
// FRONT of the profile every cell is 0: E and the H to the left start at 0, and the F that arrives from above was computed in the same column, a
// pad column of the lane above (a lane works on the block the lane above it left one step earlier).  In a pad column BEHIND a profile's end F starts
// at 0 at the top and is handed down inside the pad column, E comes from the real cell to the left, E = max(E_left - ge, H_left - go) < H_left: by
// induction along the pad columns and down them every such cell is 0 or strictly below a real cell of the pair.  In a pad row E starts at 0 and
// F comes down from the real cell above.  No real cell reads a pad cell: pad rows lie below the target, pad columns in front of column 0 hold zeros
// (what the recurrence puts there anyway), and pad columns behind the end lie to the right of every real cell of that half.  The halves of a
// register never mix, so the shorter profile's pad columns do not touch the longer one's cells.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/metaeuk_amd.h"
#include "mk_align.hpp"
#include "mk_filters.hpp"

namespace mk {

constexpr int GAP_OPEN = 11, GAP_EXTEND = 1, GAP_SCORE_CAP = 32767, GAP_PAD = -32768;
// the kernel's work split (mk_gapped.hip): lanes per target, rows per lane of the three tile shapes (a tile is GAP_GROUP x rows), queries per
// register, blocks of 256 / GAP_GROUP targets a workgroup walks with one image, the budget of the score array
constexpr int GAP_GROUP = 8, GAP_SHAPES = 3, GAP_PACK = 2, GAP_BLOCKS_PER_WG = 4;
__host__ __device__ constexpr int gapped_shape_rows(int shape) { return shape == 0 ? 4 : (shape == 1 ? 8 : 16); }
constexpr int GAP_MAX_TILE = GAP_GROUP * gapped_shape_rows(GAP_SHAPES - 1);
constexpr uint64_t GAP_SCORE_BUDGET = 256ull << 20;
constexpr uint64_t GAP_PARK_BUDGET = 128ull << 20;        // device scratch for the parked bottom rows of queries beyond the largest tile
constexpr uint32_t gapped_park_strips() { return (256 / GAP_GROUP) * GAP_BLOCKS_PER_WG; }
constexpr int GAP_PAD_CODE = 21;                          // the image line of a column outside the target

// the arithmetic of one cell for a value type: int on the host, two int16 halves in the kernel
struct GapInt {
    typedef int V;
    static __host__ __device__ int adds(int a, int b) { const int s = a + b; return s > GAP_SCORE_CAP ? GAP_SCORE_CAP : (s < -32768 ? -32768 : s); }
    static __host__ __device__ int subs0(int a, int b) { return a > b ? a - b : 0; }
    static __host__ __device__ int vmax(int a, int b) { return a > b ? a : b; }
};
// the Gotoh cell step.  diag = H(i-1, j-1), s = what the cell adds (GAP_PAD for a pad row or column), E = this row's horizontal gap state,
// F = the vertical one handed down the column; all >= 0 on entry except s.  Returns H(i, j) and leaves E(i, j+1), F(i+1, j)
template <class A>
__host__ __device__ inline typename A::V gapped_cell(typename A::V diag, typename A::V s, typename A::V &E, typename A::V &F, typename A::V go, typename A::V ge) {
    const typename A::V h = A::vmax(A::vmax(A::adds(diag, s), E), F);
    const typename A::V ho = A::subs0(h, go);
    E = A::vmax(A::subs0(E, ge), ho);
    F = A::vmax(A::subs0(F, ge), ho);
    return h;
}
// what a real cell adds: matrix entry + the row's composition bias (ssw_init's word profile, score bias 0)
__host__ __device__ inline int gapped_cell_score(int matScore, int compBias) { return matScore + compBias; }

// what column `col` ([32] int8, mk_profile.hpp) of a profile query scores for residue code `code`: X and every code above it score 0
__host__ __device__ inline int gapped_profile_score(const int8_t *col, int code) { return code < 20 ? (int) col[code] : 0; }

// the pair's verdict in front of the score (Util::canBeCovered) ...
__host__ __device__ inline bool gapped_pair_scored(float covThr, int covMode, uint32_t qLen, uint32_t tLen) {
    return can_be_covered(covThr, covMode, (float) qLen, (float) tLen);
}
// ... and behind it: score > --min-ungapped-score, and the e-value verdict of the query length's gate entry (gate == nullptr: no e-value test)
__host__ __device__ inline bool gapped_evalue_passes(int score, const GateEntry &g) {
    return score >= g.s0 || (score < 256 && ((g.mask[score >> 5] >> (score & 31)) & 1u));
}
__host__ __device__ inline bool gapped_hit_kept(int score, int minUngappedScore, const GateEntry *g) {
    return score > minUngappedScore && (!g || gapped_evalue_passes(score, *g));
}
// hit_t::compareHitsByScoreAndId as one ascending 47-bit key: (32767 - score) above the rank of the DB key among the database's keys
__host__ __device__ inline uint64_t gapped_hit_key(uint32_t score, uint32_t keyRank) { return ((uint64_t) ((uint32_t) GAP_SCORE_CAP - score) << 32) | keyRank; }
constexpr int GAP_KEY_BITS = 47;

// one pair, the plain row loop in 32-bit integers (the twin).  mat = 21 x 21 int8, bias8 = the query's composition bias or nullptr
inline int gapped_pair_host(const int8_t *mat, const uint8_t *q, const int8_t *bias8, int qLen, const uint8_t *t, int tLen) {
    if (tLen <= 0) return 0;
    int *H = new int[2 * (size_t) tLen](), *F = H + tLen;          // H(i-1, .) and F(i, .) of the row above
    int best = 0;
    for (int i = 0; i < qLen; i++) {
        const int qc = q[i] < 20 ? q[i] : 20, cb = bias8 ? bias8[i] : 0;
        int diag = 0, E = 0;
        for (int j = 0; j < tLen; j++) {
            const int tc = t[j] < 20 ? t[j] : 20;
            const int h = gapped_cell<GapInt>(diag, gapped_cell_score(mat[tc * 21 + qc], cb), E, F[j], GAP_OPEN, GAP_EXTEND);
            diag = H[j]; H[j] = h;
            best = h > best ? h : best;
        }
    }
    delete[] H;
    return best;
}

// one (profile, target) pair, the same row loop over the profile's columns (the twin of the profile kernels).  aln32 = [nCols][32] int8
inline int gapped_profile_pair_host(const int8_t *aln32, int nCols, const uint8_t *t, int tLen) {
    if (tLen <= 0) return 0;
    int *H = new int[2 * (size_t) tLen](), *F = H + tLen;
    int best = 0;
    for (int i = 0; i < nCols; i++) {
        int diag = 0, E = 0;
        for (int j = 0; j < tLen; j++) {
            const int h = gapped_cell<GapInt>(diag, gapped_profile_score(aln32 + (size_t) i * 32, t[j]), E, F[j], GAP_OPEN, GAP_EXTEND);
            diag = H[j]; H[j] = h;
            best = h > best ? h : best;
        }
    }
    delete[] H;
    return best;
}

// the work split of gapped_profile_scores_kernel (mk_gapped.hip): the target in the rows (GAP_GROUP lanes x gapped_shape_rows), the profile's columns in
// blocks of GAPP_BLOCK, lane l GAPP_BLOCK columns behind lane l - 1; the image in LDS holds the columns of GAPP_WINDOW / GAPP_BLOCK steps and the lag
constexpr int GAPP_BLOCK = 4, GAPP_LAG = (GAP_GROUP - 1) * GAPP_BLOCK, GAPP_WINDOW = 256;
constexpr int GAPP_MAX_TARGET = GAP_MAX_TILE;             // longer targets take the row-tiled kernel with the profile's columns as its rows

// ---- the kernel side (mk_gapped.hip) ----
struct GappedView {
    const uint8_t *q_res; const uint64_t *q_off; const int8_t *q_bias8; uint32_t n_queries;
    const uint32_t *q_order;                   // the batch's queries by ascending length; two neighbours share a register
    const uint8_t *t_res; const uint64_t *t_off; uint32_t n_targets;
    const uint32_t *t_order;                   // the targets by ascending length
    const int8_t *mat;                         // 21 x 21 int8 [t * 21 + q]
    float cov_thr; int cov_mode;
    uint32_t q0, nq;                           // the chunk's queries: positions [q0, q0 + nq) of q_order, q0 even
    uint32_t s0, ns;                           // the chunk's targets: positions [s0, s0 + ns) of t_order
    int16_t *scores;                           // [nq][ns] one int16 per pair, 0 for a skipped pair
    unsigned long long *work;                  // [0] algorithmic bytes, [1] cells
    const GateEntry *gate;                     // [query length] the e-value verdict per score; nullptr: no e-value test (the selection reads it)
    const int8_t *p_aln = nullptr;             // profile queries: [column][32] alignment profile, q_off the column offsets (q_res, q_bias8, mat unused)
};
// the scores of the query pairs [p0, p1) of the chunk (pair p = rows 2 p and 2 p + 1) against positions [a, b) of the chunk's targets with tile
// shape `shape`; every query of the range has at most GAP_GROUP x gapped_shape_rows(shape) residues, except with the last shape, which walks a
// longer query in row tiles and parks the bottom row of a tile in `park`: one strip of parkStride uint2 per target in flight, gapped_park_strips()
// strips for each of the `blocks` workgroups the launch is made of (0: one workgroup per work item), parkStride >= the longest target of [a, b).
// Shorter shapes take no park memory
hipError_t launch_gapped_scores(const GappedView &V, int shape, uint32_t p0, uint32_t p1, uint32_t a, uint32_t b, uint2 *park, uint64_t parkStride,
                                uint32_t blocks, hipStream_t stream);
// profile queries (V.p_aln), the target in the rows: the scores of every profile pair of the chunk against positions [a, b) of the chunk's targets,
// each of at most GAP_GROUP x gapped_shape_rows(shape) residues.  Longer targets go through launch_gapped_scores, which reads V.p_aln as well
hipError_t launch_gapped_profile_scores(const GappedView &V, int shape, uint32_t a, uint32_t b, hipStream_t stream);
// the best max_seqs hits of every query of the chunk over the chunk's targets and the candidates kept from earlier target chunks (the contract of
// UngappedSelect, over gapped_hit_key)
struct GappedSelect {
    const uint32_t *key_rank, *rank_idx; int min_score; uint32_t max_seqs;
    uint64_t *cand; uint32_t *cand_cnt; uint64_t *tmp;
    mk_hit *hits; uint32_t *hit_cnt; bool last;
};
hipError_t launch_gapped_select(const GappedView &V, const GappedSelect &S, hipStream_t stream);

}  // namespace mk
