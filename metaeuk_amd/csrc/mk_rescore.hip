// metaeuk_amd/csrc/mk_rescore.hip -- the ungapped rescoring kernel of `rescorediagonal --rescore-mode 2` (the rule: mk_rescore.hpp).
// Work split: a lane group of RESCORE_GROUP = 8 lanes owns one pair of the prefilter list (list order, so the groups of a wave read neighbouring
// hits and mostly one query); a workgroup of 256 lanes takes 32 pairs.  A diagonal is walked in sweeps of RESCORE_SWEEP = 64 cells, every lane a
// contiguous segment of RESCORE_SEG = 8 cells: the diagonal of an ORF fragment against a protein is ~10^2 cells, two sweeps of 8 lanes; 16 lanes
// would idle half the group on the second sweep of most pairs and halve the pairs per wave.
// Data movement: the 21 x 21 matrix lies in LDS as 21 rows of 32 bytes (one read per cell, the row a shift); the residues of a segment come as
// three aligned dwords per side, shifted into place with v_alignbyte (query and target starts differ mod 4 in general), and only the dwords
// that begin before the segment's end are loaded.  A per-query image indexed by target code and query position was weighed against this and
// left out: it costs 21 LDS writes per query residue and a prefilter list of ORF fragments holds a handful of hits.
// Combining the lanes, all in DPP (row_shr scans masked to the 8-lane group; quad_perm and row_half_mirror butterflies), no LDS round trip:
//   prefix sum of the segment totals; prefix minimum of P carrying the LATEST position among equal minima; then every lane walks its cells with
//   RescoreState::step from (sum, minimum) in front of its segment, and the group takes the maximum of s carrying the FIRST position among equal
//   maxima.  Values and positions travel as separate 32-bit registers ((value, position) compared lexicographically): |P| reaches 2^17 * 2^4, a
//   packed 32-bit key has no room for a 17-bit position beside it, and two registers cost one more DPP move per step, less than 64-bit compares.
// Between sweeps the group carries (running sum, running minimum + position, best + positions); a later sweep or a later real diagonal replaces
// the best only when strictly greater.  Sequences of 32768 residues and more need no path of their own: the loop over the real diagonals
// a 16-bit value stands for (mk_rescore.hpp: rescore_candidate) runs for every pair, and has one crossing diagonal for short sequences.
// Identities: a second sweep over [start, end], lane k the cells k, k + 8, ..., and a group sum.
#include "mk_rescore.hpp"
#include "mk_kernels.hpp"

namespace mk {
namespace {

constexpr int G = RESCORE_GROUP, W = RESCORE_SEG;
constexpr int PAIRS_PER_BLOCK = 256 / G;
static_assert(G == 8 && W == 8, "the DPP patterns and the three-dword fetch below are written for 8 lanes x 8 cells");

template <int CTRL>
__device__ __forceinline__ int dpp(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xF, 0xF, false); }
// value of the lane D places below in the 8-lane group, `ident` for the first D lanes
template <int D>
__device__ __forceinline__ int group_shr(int v, int ident, int sub) { const int s = dpp<0x110 + D>(ident, v); return sub >= D ? s : ident; }
// butterfly partners inside the 8-lane group: lane ^ 1, lane ^ 2 (quad_perm), 7 - lane (row_half_mirror)
template <int STEP>
__device__ __forceinline__ int group_partner(int v) {
    if constexpr (STEP == 0) return dpp<0xB1>(v, v);         // quad_perm [1, 0, 3, 2]
    else if constexpr (STEP == 1) return dpp<0x4E>(v, v);    // quad_perm [2, 3, 0, 1]
    else return dpp<0x141>(v, v);                            // row_half_mirror
}
__device__ __forceinline__ int group_sum(int v) {
    v += group_partner<0>(v); v += group_partner<1>(v); v += group_partner<2>(v);
    return v;
}
// minimum of P with the LATEST position among equal minima
__device__ __forceinline__ void min_latest(int &val, int &pos, int oVal, int oPos) {
    const bool take = oVal < val || (oVal == val && oPos > pos);
    val = take ? oVal : val; pos = take ? oPos : pos;
}
// maximum of s with the FIRST end among equal maxima
__device__ __forceinline__ void max_first(int &val, int &end, int &start, int oVal, int oEnd, int oStart) {
    const bool take = oVal > val || (oVal == val && oEnd < end);
    val = take ? oVal : val; end = take ? oEnd : end; start = take ? oStart : start;
}

// the W residues at p[0 .. n) (n <= W valid, the rest unspecified) as two dwords: aligned loads, none that begins at or behind p + n
__device__ __forceinline__ void fetch8(const uint8_t *p, int n, uint32_t &lo, uint32_t &hi) {
    const uintptr_t a = (uintptr_t) p, base = a & ~(uintptr_t) 3;
    const uint32_t *w = (const uint32_t *) base;
    const uintptr_t end = a + (uintptr_t) n;
    const uint32_t d0 = w[0], d1 = base + 4 < end ? w[1] : 0u, d2 = base + 8 < end ? w[2] : 0u;
    const uint32_t sh = (uint32_t) (a & 3);
    lo = __builtin_amdgcn_alignbyte(d1, d0, sh);
    hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
}

__global__ __launch_bounds__(256) void rescore_kernel(RescoreView V) {
    __shared__ int8_t sMat[21 * 32];
    __shared__ unsigned long long sWork[2];
    for (int k = threadIdx.x; k < 21 * 32; k += 256) sMat[k] = (k & 31) < 21 ? V.mat[(k >> 5) * 21 + (k & 31)] : (int8_t) 0;
    if (threadIdx.x < 2) sWork[threadIdx.x] = 0;
    __syncthreads();
    const int sub = threadIdx.x & (G - 1);
    const uint64_t p = (uint64_t) blockIdx.x * PAIRS_PER_BLOCK + (threadIdx.x / G);
    if (p < V.n_pairs) {
        uint32_t lo = 0, hi = V.n_queries;                       // largest q with hit_off[q] <= p
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (V.hit_off[mid] <= p) lo = mid; else hi = mid; }
        const uint32_t qi = lo, ti = V.hits[p].seq_id, d16 = V.hits[p].diagonal;
        bool pass = false;
        if (sub == 0) { V.raw[p].pair = (uint32_t) p; V.pass[p] = 0; }
        if (ti >= V.n_targets) { if (sub == 0) atomicAdd(&V.flags[1], 1u); }
        else {
            const uint32_t qLen = (uint32_t) (V.q_off[qi + 1] - V.q_off[qi]), tLen = (uint32_t) (V.t_off[ti + 1] - V.t_off[ti]);
            const uint8_t *qSeq = V.q_res + V.q_off[qi], *tSeq = V.t_res + V.t_off[ti];
            // Util::canBeCovered comes before any scoring (rescorediagonal.cpp:211)
            if (can_be_covered(V.crit.filter.cov_thr, V.crit.filter.cov_mode, (float) qLen, (float) tLen)) {
                RescoreBest best;
                bool crossed = false;
                uint32_t cells = 0;
                const uint32_t nCand = rescore_candidates(qLen, tLen);
                for (uint32_t k = 0; k < nCand; k++) {
                    const int real = rescore_candidate(k, d16, tLen);
                    const RescoreDiag g = rescore_geometry(real, qLen, tLen);
                    if (g.len == 0) continue;
                    crossed = true; cells += g.len;
                    RescoreState carry;                           // the group's state in front of the sweep (the same in all eight lanes)
                    for (uint32_t base = 0; base < g.len; base += RESCORE_SWEEP) {
                        const uint32_t i0 = base + (uint32_t) sub * W;
                        const int n = i0 < g.len ? (int) min((uint32_t) W, g.len - i0) : 0;
                        int c[W];
                        if (n > 0) {
                            uint32_t ql, qh, tl, th;
                            fetch8(qSeq + g.q0 + i0, n, ql, qh);
                            fetch8(tSeq + g.t0 + i0, n, tl, th);
#pragma unroll
                            for (int j = 0; j < W; j++) {
                                const uint32_t qc = ((j < 4 ? ql : qh) >> (8 * (j & 3))) & 0xFFu, tc = ((j < 4 ? tl : th) >> (8 * (j & 3))) & 0xFFu;
                                c[j] = j < n ? (int) sMat[(min(qc, 20u) << 5) + min(tc, 20u)] : 0;
                            }
                        } else {
#pragma unroll
                            for (int j = 0; j < W; j++) c[j] = 0;
                        }
                        // segment total and the latest minimum of the segment's own prefix sums
                        int tot = 0, mVal = 0x7FFFFFFF, mPos = -1;
#pragma unroll
                        for (int j = 0; j < W; j++) { tot += c[j]; if (j < n && tot <= mVal) { mVal = tot; mPos = (int) i0 + j; } }
                        // inclusive scan of the totals over the group -> the sum in front of this lane's segment
                        int inc = tot;
                        inc += group_shr<1>(inc, 0, sub); inc += group_shr<2>(inc, 0, sub); inc += group_shr<4>(inc, 0, sub);
                        const int before = carry.sum + (inc - tot);
                        if (n > 0) mVal += before;               // now a value of P
                        // inclusive scan of the minima (latest among equals), then one lane down: the minimum of P in front of the segment
                        int sVal = mVal, sPos = mPos;
                        min_latest(sVal, sPos, group_shr<1>(sVal, 0x7FFFFFFF, sub), group_shr<1>(sPos, -1, sub));
                        min_latest(sVal, sPos, group_shr<2>(sVal, 0x7FFFFFFF, sub), group_shr<2>(sPos, -1, sub));
                        min_latest(sVal, sPos, group_shr<4>(sVal, 0x7FFFFFFF, sub), group_shr<4>(sPos, -1, sub));
                        RescoreState s;
                        s.sum = before; s.minVal = carry.minVal; s.minPos = carry.minPos;
                        min_latest(s.minVal, s.minPos, group_shr<1>(sVal, 0x7FFFFFFF, sub), group_shr<1>(sPos, -1, sub));
#pragma unroll
                        for (int j = 0; j < W; j++) if (j < n) s.step(c[j], (int) i0 + j);
                        // the group's maximum (first end among equals), total and minimum (latest among equals): butterflies
                        int bVal = s.best, bEnd = s.best > 0 ? s.bestEnd : 0x7FFFFFFF, bStart = s.bestStart;
                        max_first(bVal, bEnd, bStart, group_partner<0>(bVal), group_partner<0>(bEnd), group_partner<0>(bStart));
                        max_first(bVal, bEnd, bStart, group_partner<1>(bVal), group_partner<1>(bEnd), group_partner<1>(bStart));
                        max_first(bVal, bEnd, bStart, group_partner<2>(bVal), group_partner<2>(bEnd), group_partner<2>(bStart));
                        if (bVal > carry.best) { carry.best = bVal; carry.bestEnd = bEnd; carry.bestStart = bStart; }
                        carry.sum += group_sum(tot);
                        min_latest(mVal, mPos, group_partner<0>(mVal), group_partner<0>(mPos));
                        min_latest(mVal, mPos, group_partner<1>(mVal), group_partner<1>(mPos));
                        min_latest(mVal, mPos, group_partner<2>(mVal), group_partner<2>(mPos));
                        if (mVal <= carry.minVal) { carry.minVal = mVal; carry.minPos = mPos; }      // (every position of this sweep is later)
                    }
                    rescore_offer(best, carry, real);
                }
                if (!crossed) { if (sub == 0) atomicAdd(&V.flags[1], 1u); }
                else {
                    // identities over [start, end] of the winning diagonal
                    int ids = 0;
                    if (best.found) {
                        const RescoreDiag g = rescore_geometry(best.real, qLen, tLen);
                        for (int i = best.start + sub; i <= best.end; i += G) ids += qSeq[g.q0 + (uint32_t) i] == tSeq[g.t0 + (uint32_t) i] ? 1 : 0;
                    }
                    ids = group_sum(ids);
                    if (sub == 0) {
                        if ((uint32_t) best.score >= V.smax || qLen > V.maxLen || V.lenIdx[qLen] < 0) atomicAdd(&V.flags[0], 1u);
                        else {
                            mk_alignment a;
                            pass = rescore_record(V.crit, best, ti, (int) qLen, (int) tLen, ids, V.evalTab[(size_t) V.lenIdx[qLen] * V.smax + (uint32_t) best.score],
                                                  V.bitScore[best.score], a);
                            V.rec[p] = a; V.pass[p] = pass ? 1 : 0;
                        }
                        atomicAdd(&sWork[0], (unsigned long long) (2u * cells + (uint32_t) (sizeof(mk_hit) + sizeof(mk_alignment))));
                        atomicAdd(&sWork[1], (unsigned long long) cells);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 && sWork[threadIdx.x]) atomicAdd(&V.work[threadIdx.x], sWork[threadIdx.x]);
}

}  // namespace

hipError_t launch_rescore(const RescoreView &V, hipStream_t stream) {
    if (V.n_pairs == 0) return hipSuccess;
    const uint64_t blocks = (V.n_pairs + PAIRS_PER_BLOCK - 1) / PAIRS_PER_BLOCK;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rescore_kernel, dim3((uint32_t) blocks), dim3(256), 0, stream, V);
    return hipGetLastError();
}

}  // namespace mk
