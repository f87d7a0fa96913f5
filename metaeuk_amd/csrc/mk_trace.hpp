// metaeuk_amd/csrc/mk_trace.hpp -- the backtrace of --alignment-mode 3 (Matcher::SCORE_COV_SEQID) / -a, one restatement for the host
// (mk_backtrace_host, the host assembly of the alignment stage) and the kernel of mk_trace.hip.
// SmithWaterman::banded_sw<SEQ_SEQ> (M/src/alignment/StripedSmithWaterman.cpp:1347-1600) on the rectangle [q_start..q_end] x [t_start..t_end] of
// a pair whose score and coordinates are known, then computerBacktrace<SUBSTITUTIONMATRIX> (:547-581) and Util::computeSeqId (Util.cpp:532-542).
// Kept from the reference: the first band |tn - qn| + 1, the whole DP redone with the band doubled while max < score, the three rolling
// rows h_b / e_b / h_c in BAND coordinates with their edge cells set to 0 at every row (including the cell the `edge` index names when the
// band is wider than the target, which is a cell of the previous row), the first row opening with -gap_open / -gap_extend, the strict
// comparisons (temp1 > temp2 -> open, temp1 <= temp2 -> M, e1 > f1 -> E's code), int32 cells mat[q][t] + bias8, the trace from the corner
// (qn - 1, tn - 1) in state H until (0, 0) and the final M of cell (0, 0).
// Defined here where the reference is not: the rows start every attempt as zeros (the reference mallocs e_b and h_c); a band that has reached
// max(qn, tn) without the score is TRACE_STALLED (the reference doubles until its size overflows and exits); a trace that reads a cell outside
// the band or does not stop on (0, 0) gives no path (TRACE_LEFT_BAND: the reference reads unwritten memory or returns no cigar).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

namespace mk {

// Matcher::SCORE_COV / SCORE_COV_SEQID (Matcher.h:24-26), Parameters::SEQ_ID_* (Parameters.h:285-287)
constexpr int ALIGNMENT_MODE_SCORE_COV = 2, ALIGNMENT_MODE_SCORE_COV_SEQID = 3;
constexpr int SEQ_ID_ALN_LEN = 0, SEQ_ID_SHORT = 1, SEQ_ID_LONG = 2;

constexpr int TRACE_OK = 0, TRACE_MISSED = 1 /* max < score at this band */, TRACE_LEFT_BAND = 2, TRACE_STALLED = 3;

// four direction bits per band cell: bit 0 = E opened (the reference's code 3, else 2), bit 1 = F opened (5, else 4), bits 2-3 = H: 0 M, 1 E's
// code, 2 F's code.  The reference keeps three bytes.  Eight cells share a 32-bit word, a row of the band takes trace_row_words(band) words:
// a lane stores a word per eight cells (a store per cell would put a memory wait into every cell's dependent chain).
constexpr uint32_t DIR_E_OPEN = 1, DIR_F_OPEN = 2, DIR_H_E = 4, DIR_H_F = 8;

// element k of a lane's array lives at p[k * stride]: stride 1 on the host, 64 where the lanes of a wave interleave their arrays
template <typename T>
struct Strided {
    T *p; size_t stride;
    __host__ __device__ inline T &operator[](size_t k) const { return p[k * stride]; }
};

__host__ __device__ inline int trace_first_band(int qn, int tn) { return (tn > qn ? tn - qn : qn - tn) + 1; }
// cells one attempt at `band` computes: row i covers the columns max(0, i - band) .. min(tn - 1, i + band)
__host__ __device__ inline uint64_t trace_band_cells(int qn, int tn, int band) {
    uint64_t c = 0;
    for (int i = 0; i < qn; i++) {
        const int beg = i - band > 0 ? i - band : 0, end = i + band < tn - 1 ? i + band : tn - 1;
        if (end >= beg) c += (uint64_t) (end - beg + 1);
    }
    return c;
}
// direction words per row (2 * band + 1 cells of four bits), direction bytes of one attempt and ints per rolling row (2 * band + 3)
__host__ __device__ inline uint64_t trace_row_words(int band) { return (2ull * (uint64_t) band + 1ull + 7ull) / 8ull; }
__host__ __device__ inline uint64_t trace_dir_bytes(int qn, int band) { return (uint64_t) qn * trace_row_words(band) * 4ull; }
__host__ __device__ inline uint64_t trace_row_ints(int band) { return 2ull * (uint64_t) band + 3ull; }

// one attempt of banded_sw's do-loop body: fills `dir`, returns max.  hb / eb / hc hold trace_row_ints(band) ints each.
// The band indices of the reference's set_u: a cell (i, j) is u = j - x + 1 of its own row (x = max(i - band, 0)) and e = j - xp + 1 of the
// row above (xp = max(i - 1 - band, 0)); its left neighbour is b = u - 1 and its diagonal neighbour d = e - 1.  So h_c[b] is the H this lane
// just computed (h_c[0] = 0 for the first cell of a row) and h_b[d] is the h_b[e] it read one cell earlier -- h_b is not written inside a row --
// and both stay in registers.  h_b[e] / e_b[e] of the NEXT cell are read before this cell's stores (e(j + 1) - u(j) is
// 1 or 2 and no earlier cell of the row has written index e(j + 1): the values are those the reference reads), which takes the loads off
// the dependent chain of a cell.
// Target residues and scores are taken eight cells at a time: the residues of the next block of the row (and of the first block of the next row,
// with that row's query residue and bias) are loaded while this block is computed, the eight scores of a block are looked up together -- a lane
// walks its cells alone, so every load left inside a cell would be paid in full, cell after cell.  (Indices past the row's end are clamped to
// the rectangle's last column and never used.)
template <class Rows, class Dirs>
__host__ __device__ inline int32_t banded_fill(const int8_t *mat, const uint8_t *q, const int8_t *bias8, int qn, const uint8_t *t, int tn,
                                               int gapOpen, int gapExtend, int band, Rows hb, Rows eb, Rows hc, Dirs dir) {
    const int64_t width = (int64_t) band * 2 + 3;
    const uint64_t rowWords = trace_row_words(band);
    int32_t max = 0;
    for (int64_t k = 0; k < width; k++) { hb[k] = 0; eb[k] = 0; hc[k] = 0; }
    uint32_t rowT[8];                                                 // residues of the first block of row i
#pragma unroll
    for (int k = 0; k < 8; k++) rowT[k] = t[k < tn - 1 ? k : tn - 1];
    uint32_t qc = q[0];
    int32_t bias = bias8[0];
    for (int i = 0; i < qn; i++) {
        int beg = 0, end = tn - 1, u = 0;
        int j = i - band; beg = beg > j ? beg : j;
        j = i + band; end = end < j ? end : j;
        const int64_t edge = end + 1 < width - 1 ? end + 1 : width - 1;
        int32_t f = 0;
        hb[0] = 0; eb[0] = 0; hb[edge] = 0; eb[edge] = 0; hc[0] = 0;
        uint32_t nextT[8], qcN = 0;
        int32_t biasN = 0;
        if (i + 1 < qn) {
            const int begN = i + 1 - band > 0 ? i + 1 - band : 0;
#pragma unroll
            for (int k = 0; k < 8; k++) nextT[k] = t[begN + k < tn - 1 ? begN + k : tn - 1];
            qcN = q[i + 1]; biasN = bias8[i + 1];
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) nextT[k] = 0;
        }
        uint64_t word = rowWords * (uint64_t) i;                      // (i, beg) is column 0 of the row's directions: beg == x
        uint32_t acc = 0, col = 0;
        const int8_t *mrow = mat + (int) qc * 21;
        const int x = i - band > 0 ? i - band : 0, xp = i - 1 - band > 0 ? i - 1 - band : 0;
        int32_t hLeft = 0;                                            // h_c[b] of the first cell: h_c[0]
        int32_t hDiag = hb[(size_t) (beg - xp)];                      // h_b[d] of the first cell
        int32_t hUp = hb[(size_t) (beg - xp + 1)], eUp = eb[(size_t) (beg - xp + 1)];     // h_b[e], e_b[e] (row 0: zeros nobody uses)
        uint32_t tb[8];
#pragma unroll
        for (int k = 0; k < 8; k++) tb[k] = rowT[k];
        for (int j0 = beg; j0 <= end; j0 += 8) {
            uint32_t tbN[8];
            int32_t sc[8];
#pragma unroll
            for (int k = 0; k < 8; k++) tbN[k] = t[j0 + 8 + k < end ? j0 + 8 + k : end];
#pragma unroll
            for (int k = 0; k < 8; k++) sc[k] = (int32_t) mrow[tb[k]] + bias;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                j = j0 + k;
                if (j <= end) {
                    int32_t hUpN = 0, eUpN = 0;
                    if (j < end) { hUpN = hb[(size_t) (j - xp + 2)]; eUpN = eb[(size_t) (j - xp + 2)]; }
                    u = j - x + 1;
                    uint32_t code = 0;
                    int32_t temp1 = i == 0 ? -gapOpen : hUp - gapOpen;
                    int32_t temp2 = i == 0 ? -gapExtend : eUp - gapExtend;
                    const int32_t ev = temp1 > temp2 ? temp1 : temp2;
                    eb[(size_t) u] = ev;
                    if (temp1 > temp2) code |= DIR_E_OPEN;
                    temp1 = hLeft - gapOpen;
                    temp2 = f - gapExtend;
                    if (temp1 > temp2) code |= DIR_F_OPEN;
                    f = temp1 > temp2 ? temp1 : temp2;
                    const int32_t f1 = f > 0 ? f : 0;
                    const int32_t e1 = ev > 0 ? ev : 0;
                    temp1 = e1 > f1 ? e1 : f1;
                    temp2 = hDiag + sc[k];
                    const int32_t h = temp1 > temp2 ? temp1 : temp2;
                    hc[(size_t) u] = h;
                    if (h > max) max = h;
                    if (!(temp1 <= temp2)) code |= e1 > f1 ? DIR_H_E : DIR_H_F;
                    acc |= code << (4u * (col & 7u));
                    col++;
                    if ((col & 7u) == 0u || j == end) { dir[word++] = acc; acc = 0; }
                    hLeft = h; hDiag = hUp; hUp = hUpN; eUp = eUpN;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) tb[k] = tbN[k];
        }
        for (j = 1; j <= u; j++) hb[(size_t) j] = hc[(size_t) j];
#pragma unroll
        for (int k = 0; k < 8; k++) rowT[k] = nextT[k];
        qc = qcN; bias = biasN;
    }
    return max;
}

// the trace over the directions of the attempt that reached the score.  ops (may be null): the uncompressed operations are written BACKWARDS
// from opsEnd[-1]; the string is opsEnd[-btLen .. 0).  TRACE_OK or TRACE_LEFT_BAND (then *btLen = *identities = 0).
template <class Dirs, class Ops>
__host__ __device__ inline int banded_trace(const uint8_t *q, int qn, const uint8_t *t, int tn, int band, Dirs dir, Ops opsEnd, bool writeOps,
                                            uint32_t opsCap, uint32_t *btLen, uint32_t *identities) {
    const uint64_t rowWords = trace_row_words(band);
    int i = qn - 1, j = tn - 1, state = 2;   // 0 e, 1 f, 2 h
    uint32_t n = 0, ids = 0;
    *btLen = 0; *identities = 0;
    while (i > 0 || j > 0) {
        if (i < 0 || j < 0) return TRACE_LEFT_BAND;
        const int beg = i - band > 0 ? i - band : 0, end = i + band < tn - 1 ? i + band : tn - 1;
        if (j < beg || j > end) return TRACE_LEFT_BAND;
        const uint32_t code = (dir[rowWords * (uint64_t) i + (uint64_t) ((j - beg) >> 3)] >> (4u * ((uint32_t) (j - beg) & 7u))) & 15u;
        // the reference's code of the cell in this state: 1 M, 2 E extended, 3 E opened, 4 F extended, 5 F opened
        int c;
        if (state == 0) c = (code & DIR_E_OPEN) ? 3 : 2;
        else if (state == 1) c = (code & DIR_F_OPEN) ? 5 : 4;
        else c = (code & DIR_H_E) ? ((code & DIR_E_OPEN) ? 3 : 2) : (code & DIR_H_F) ? ((code & DIR_F_OPEN) ? 5 : 4) : 1;
        char op;
        switch (c) {
            case 1: ids += (uint32_t) (q[i] == t[j]); --i; --j; state = 2; op = 'M'; break;
            case 2: --i; state = 0; op = 'I'; break;
            case 3: --i; state = 2; op = 'I'; break;
            case 4: --j; state = 1; op = 'D'; break;
            default: --j; state = 2; op = 'D'; break;
        }
        if (n + 1 >= opsCap) return TRACE_LEFT_BAND;          // (a monotone path has at most qn + tn - 1 operations: never on a path that ends on (0, 0))
        n++;
        if (writeOps) opsEnd[-(int64_t) n] = op;
    }
    if (i != 0 || j != 0) return TRACE_LEFT_BAND;
    ids += (uint32_t) (q[0] == t[0]);                         // the final M of cell (0, 0)
    n++;
    if (writeOps) opsEnd[-(int64_t) n] = 'M';
    *btLen = n; *identities = ids;
    return TRACE_OK;
}

// Util::computeSeqId (Util.cpp:532-542): float division in the reference's order
__host__ __device__ inline float compute_seq_id(int seqIdMode, int aaIds, int qLen, int tLen, int alnLen) {
    if (seqIdMode == SEQ_ID_ALN_LEN) return static_cast<float>(aaIds) / static_cast<float>(alnLen);
    if (seqIdMode == SEQ_ID_SHORT) return static_cast<float>(aaIds) / static_cast<float>(qLen < tLen ? qLen : tLen);
    return static_cast<float>(aaIds) / static_cast<float>(qLen > tLen ? qLen : tLen);
}

// ---- the kernel side (mk_trace.hip) ----
// One banded DP + trace: the rectangle starts at q_res[q_pos] / t_res[t_pos].  `ops_end` = end of the pair's region in the ops buffer.
struct TraceJob { uint64_t t_pos, q_pos, ops_end; int32_t qn, tn, score, band; uint32_t slot, pad; };
struct TraceOut { uint32_t bt_len, identities; int32_t status; int32_t pad; };
// Jobs are taken 64 to a workgroup (one lane each); group g's direction bytes start at dir_base[g] (64 interleaved columns).  A launch is of
// one class: lds_width > 0 -- every job has 2 * band + 3 <= lds_width and the three rolling rows are per-lane LDS columns (11 ints: band <= 4,
// 8 KB of LDS per workgroup of 64 lanes; 23: band <= 10, 17 KB; 67: band <= 32, 50 KB; 259: band <= 128, 16 lanes, 49 KB; 1027: band <= 512, 4
// lanes, 48 KB); lds_width == 0 -- the rows in global scratch: group g's three rows at row_base[g] ints into `rows` (row_base has a closing entry).
constexpr int TRACE_NCLASS = 6;
constexpr int TRACE_LDS_WIDTH = 1027;
__host__ __device__ inline int trace_class_width(int c) { const int w[TRACE_NCLASS] = {11, 23, 67, 259, 1027, 0}; return w[c]; }
__host__ __device__ inline int trace_class_lanes(int c) { const int l[TRACE_NCLASS] = {64, 64, 64, 16, 4, 64}; return l[c]; }
struct TraceLaunch {
    const uint8_t *q_res; const int8_t *q_bias8; const uint8_t *t_res; const int8_t *mat;     // mat[q * 21 + t]
    const TraceJob *jobs; TraceOut *out; uint32_t n_jobs;
    uint32_t lds_width;
    uint32_t lanes;              // jobs per workgroup and stride of the interleaving: the class's, or 1 for a pair too large to interleave (global rows only)
    const uint64_t *dir_base; uint32_t *dirs;    // dir_base in words
    const uint64_t *row_base; int32_t *rows;       // wide launch only
    char *ops; uint32_t write_ops;
    int gap_open, gap_extend;
};
hipError_t launch_trace(const TraceLaunch &L, hipStream_t stream);

// ---- the stage: every rectangle through the kernel, band by band ----
// A rectangle starts at q_res[q_pos] / t_res[t_pos] (device arrays) and has qn x tn cells; score = the pair's Smith-Waterman score.
struct TracePair { uint64_t q_pos, t_pos; int32_t qn, tn, score; };
struct TraceResult { uint32_t bt_len, identities, attempts; int32_t status /* TRACE_OK / TRACE_LEFT_BAND */, band /* of the last attempt */; };
// Scratch of one launch (direction bytes + wide rows + operation bytes) stays under this; a single pair that needs more: MK_ERR_UNSUPPORTED.
constexpr uint64_t TRACE_SLICE_BYTES = 512ull << 20;
struct TraceStageStats { double cells = 0; uint64_t launches = 0, jobs[TRACE_NCLASS] = {0, 0, 0, 0, 0, 0}, leftBand = 0; };
typedef int (*trace_timed_begin_fn)(const char *name, double bytes, double cells);
typedef void (*trace_timed_end_fn)(int handle);
// Rounds: all pairs at their first band; those that miss the score again with the band doubled (one readback per launch).  keepOps: the
// operation strings, pair p's at ops[opsOff[p] .. opsOff[p] + res[p].bt_len) with opsOff[p + 1] - opsOff[p] >= qn + tn (host arrays).
// MK_OK, MK_ERR_SW_MISMATCH (a stalled band), MK_ERR_UNSUPPORTED (a pair beyond TRACE_SLICE_BYTES), MK_ERR_DEVICE.
int run_trace_device(const uint8_t *dQRes, const int8_t *dQBias8, const uint8_t *dTRes, const int8_t *dMat, const TracePair *pairs, size_t n,
                     int gapOpen, int gapExtend, bool keepOps, const uint64_t *opsOff, char *ops, hipStream_t stream, TraceResult *res,
                     std::string &err, trace_timed_begin_fn tb, trace_timed_end_fn te, TraceStageStats *stats = nullptr);
// the same pair on the host: banded_sw + computerBacktrace as one call (pointers at the rectangle's first residues).  ops (may be null)
// receives the string from ops[0]; opsCap >= qn + tn.
int trace_host(const int8_t *mat, const uint8_t *q, const int8_t *bias8, int qn, const uint8_t *t, int tn, int score, int gapOpen, int gapExtend,
               char *ops, uint32_t opsCap, TraceResult *res);


}  // namespace mk
