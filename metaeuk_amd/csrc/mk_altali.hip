// metaeuk_amd/csrc/mk_altali.hip -- the alternative-alignment kernel of `align` / `search --alt-ali N` (the rule: mk_altali.hpp).
// Work split: a job is one open chain = (query, target, the chain's intervals).  One fused kernel per job: forward pass, e-value / coverage
// gate from the host's table, reverse pass over the prefix in front of the end cell, record and verdict by the group's first lane, which also
// appends the accepted interval to the chain.  The jobs of a round are few beside the score pass of the stage (one per accepted record) and
// independent, so nothing is shared between them.  Two lane shapes, both ALTALI_R = 8 rows per lane in registers:
//   8 lanes  x 8 rows  queries of at most 64 rows (ORF fragments): eight jobs per wave, every group on its own profile;
//   64 lanes x 8 rows  longer queries in row tiles of 512; the bottom row of a tile is parked in HBM (4 B per column, a slot handed out by
//                      a counter) and read back by lane 0 of the next tile.
// Recurrence: plain Gotoh, the anti-diagonal wavefront of mk_sw.hip (lane l is on column s - l at step s; H of the lane's last row, the running
// F and the residue travel one lane up per step by DPP), int32 cells saturating at 32 767, the packed key (score << 17 | ~column) per row.
// Data movement: the query profile prof[residue][row] is built in LDS per pass and tile from the staged residues and bias and the LDS copy of
// the matrix (the reverse pass is the same build with the rows counted down from the end cell).  The chain's intervals sit in LDS beside it.
// The target comes as ALIGNED DWORDS, one per lane and block (32 columns on 8 lanes, 256 on 64), two blocks ahead of their use; the mask is
// applied ON THE FETCH: a dword whose four target positions miss the hull of the intervals is taken as loaded (two compares), one that meets
// it gets 20 substituted byte by byte by the exact test of mk_altali.hpp.  The reverse pass loads the dwords downwards and swaps their bytes,
// so a step reads byte (u & 3) of the dword of lane (u >> 2) in both directions (one ds_bpermute per step), u = the column + the start's
// offset in its dword.  No masked copy of a target exists in HBM.
// One wave per workgroup: the LDS writes are ordered by wavefront fences behind the loops that write, none at a loop head.
#include "mk_altali.hpp"
#include "mk_align.hpp"
#include "mk_kernels.hpp"

namespace mk {
namespace {

constexpr int R = ALTALI_R;

// value of lane - 1 of the G-lane group, `top` for the group's first lane
template <int G>
__device__ __forceinline__ uint32_t lane_up(uint32_t top, uint32_t x, int lane) {
    const uint32_t v = (uint32_t) __builtin_amdgcn_update_dpp((int) top, (int) x, G == 8 ? 0x111 /* row_shr:1 */ : 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    return lane == 0 ? top : v;
}
__device__ __forceinline__ int max3(int a, int b, int c) { return max(max(a, b), c); }
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// one pass of one job on a G-lane group.  Rows: query residues qBase + k * qDir, k < rows; columns: target positions tFirst + c * tDir, c < cols
// (positions of the target, the mask's coordinates).  Returns in every lane of the group the key of the maximum and its row.
template <int G>
__device__ __forceinline__ void altali_pass(const AltView &V, int8_t *prof, const int8_t *sMat, const AltInterval *iv, int nIv, int hullLo, int hullHi,
                                            int lane, int64_t qBase, int qDir, int rows, int64_t tOff, int tLen, int tFirst, int tDir, int cols,
                                            uint32_t *border, int &score, int &endCol, int &endRow) {
    constexpr int ROWS = G * R;
    const int go = V.crit.gapOpen, ge = V.crit.gapExtend;
    const int nTiles = (rows + ROWS - 1) / ROWS;
    // the aligned dword stream: u = column + a0 counts bytes from the dword that holds the first column, in pass direction
    const int64_t absFirst = tOff + tFirst;
    const int a0 = tDir > 0 ? (int) (absFirst & 3) : 3 - (int) (absFirst & 3);
    const int64_t dwFirst = absFirst >> 2;
    const uint32_t *tWords = reinterpret_cast<const uint32_t *>(V.t_res);
    const auto load_block = [&](int blk) -> uint32_t {
        const int64_t dw = dwFirst + (int64_t) tDir * ((int64_t) blk * G + lane);
        const int64_t b0 = dw * 4;
        if (dw < 0 || b0 >= tOff + tLen || b0 + 4 <= tOff) return 0u;         // no byte of this target in it: not loaded
        uint32_t w = tWords[dw];
        const int p0 = (int) (b0 - tOff);                                       // target position of byte 0
        if (p0 < hullHi && p0 + 4 > hullLo) {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (altali_masked(iv, nIv, p0 + j)) w = (w & ~(0xFFu << (8 * j))) | (ALTALI_X << (8 * j));
        }
        return tDir > 0 ? w : __builtin_bswap32(w);
    };
    uint32_t bestKey = 0;
    int bestRow = 0;
    for (int tile = 0; tile < nTiles; tile++) {
        const int row0 = tile * ROWS;
        // ---- the profile of the tile: residues and bias staged, then prof[t][row] = mat[t][q] + bias (int8), rows behind the query and code 21 zero
        uint8_t *sQ = reinterpret_cast<uint8_t *>(prof) + 22 * ROWS;
        int8_t *sB = reinterpret_cast<int8_t *>(sQ) + ROWS;
        for (int row = lane; row < ROWS; row += G) {
            const bool real = row0 + row < rows;
            const int64_t qi = qBase + (int64_t) (real ? row0 + row : 0) * qDir;
            sQ[row] = real ? V.q_res[qi] : (uint8_t) 255;
            sB[row] = real ? V.q_bias8[qi] : (int8_t) 0;
        }
        wave_sync_lds();
        for (int idx = lane; idx < 22 * ROWS; idx += G) {
            const int t = idx / ROWS, row = idx - t * ROWS;
            const uint32_t qc = sQ[row];
            prof[idx] = (t < 21 && qc != 255u) ? (int8_t) altali_cell(sMat, qc, (int) sB[row], (uint32_t) t) : (int8_t) 0;
        }
        wave_sync_lds();

        int H[R], E[R];
        uint32_t key[R];
#pragma unroll
        for (int r = 0; r < R; r++) { H[r] = 0; E[r] = 0; key[r] = 0; }
        uint32_t out0 = 0, out1 = 21u;           // what this lane hands to lane + 1: (H of its last row | F << 16), the residue
        int hupPrev = 0;
        const int steps = cols > 0 ? cols + G - 1 : 0;
        const bool readTop = tile > 0, writeBottom = tile + 1 < nTiles;
        uint32_t dwCur = load_block(0), dwNext = load_block(1);
        int s = 0;
        for (int blk = 0; s < steps; blk++) {
            const uint32_t dwAhead = load_block(blk + 2);
            const int sEnd = min(steps, (blk + 1) * 4 * G - a0);
            for (; s < sEnd; s++) {
                const int u = a0 + s;
                const uint32_t w = (uint32_t) __shfl((int) dwCur, (u >> 2) & (G - 1), G);
                const uint32_t top1 = s < cols ? min((w >> (8 * (u & 3))) & 0xFFu, 20u) : 21u;     // 21 = "no column": the all-zero profile row
                uint32_t top0 = 0;
                if (readTop && lane == 0 && s < cols) top0 = border[s];
                const uint32_t in0 = lane_up<G>(top0, out0, lane);
                const uint32_t tres = lane_up<G>(top1, out1, lane);
                const int hup = (int) (in0 & 0xFFFFu);
                int F = (int) (in0 >> 16);
                const int c = s - lane;
                const uint32_t cinv = 0x1FFFFu - (uint32_t) max(c, 0);
                const uint2 pw = *reinterpret_cast<const uint2 *>(prof + tres * ROWS + lane * R);
                int dsave = hupPrev;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int sc = (int) (int8_t) (((r < 4 ? pw.x : pw.y) >> (8 * (r & 3))) & 0xFFu);
                    const int d = min(dsave + sc, 32767);
                    dsave = H[r];
                    const int h = max3(d, E[r], F);
                    key[r] = max(key[r], ((uint32_t) h << 17) | cinv);
                    const int ho = h - go;
                    E[r] = max3(E[r] - ge, ho, 0);
                    F = max3(F - ge, ho, 0);
                    H[r] = h;
                }
                hupPrev = hup;
                out0 = (uint32_t) H[R - 1] | ((uint32_t) F << 16);
                out1 = tres;
                if (writeBottom && lane == G - 1 && c >= 0 && c < cols) border[c] = out0;
            }
            dwCur = dwNext; dwNext = dwAhead;
        }
#pragma unroll
        for (int r = 0; r < R; r++)
            if (key[r] > bestKey) { bestKey = key[r]; bestRow = row0 + lane * R + r; }
        wave_sync_lds();                           // the border row and the profile of this tile are done with before the next tile writes
    }
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
        const uint32_t ok = (uint32_t) __shfl_xor((int) bestKey, m, G);
        const int orow = __shfl_xor(bestRow, m, G);
        if (ok > bestKey || (ok == bestKey && orow < bestRow)) { bestKey = ok; bestRow = orow; }
    }
    score = (int) (bestKey >> 17);
    endCol = score > 0 ? (int) (0x1FFFFu - (bestKey & 0x1FFFFu)) : -1;
    endRow = score > 0 ? bestRow : -1;
}

template <int G>
__global__ __launch_bounds__(64) void altali_kernel(AltView V) {
    constexpr int ROWS = G * R, GROUPS = 64 / G;
    __shared__ __attribute__((aligned(16))) int8_t sProf[GROUPS * 24 * ROWS];     // per group: 22 profile rows + the staged residues and bias
    __shared__ int8_t sMat[448];
    __shared__ AltInterval sIv[GROUPS][ALTALI_MAX + 1];
    for (int k = (int) threadIdx.x; k < 441; k += 64) sMat[k] = V.mat[k];
    const int lane = (int) threadIdx.x % G, grp = (int) threadIdx.x / G;
    const uint32_t job = blockIdx.x * (uint32_t) GROUPS + (uint32_t) grp;
    const bool inList = job < V.n_jobs;
    const uint32_t chain = inList ? V.jobs[job] : 0u;
    uint32_t qi = 0, ti = 0;
    int qLen = 0, tLen = 0, nIv = 0;
    if (inList) {
        qi = V.chain_q[chain]; ti = V.chain_t[chain];
        qLen = (int) (V.q_off[qi + 1] - V.q_off[qi]); tLen = (int) (V.t_off[ti + 1] - V.t_off[ti]);
        nIv = (int) min(V.chain_niv[chain], V.iv_stride);
    }
    // a job runs in the lane shape of its query; the other kernel takes the rest
    const bool mine = inList && (G == 8 ? qLen <= ALTALI_SMALL_ROWS : qLen > ALTALI_SMALL_ROWS);
    if (!mine) { qLen = 0; tLen = 0; nIv = 0; }
    for (int k = lane; k < nIv; k += G) sIv[grp][k] = V.chain_iv[(size_t) chain * V.iv_stride + (uint32_t) k];
    wave_sync_lds();
    int hullLo = 0x7FFFFFFF, hullHi = -1;
    for (int k = 0; k < nIv; k++) { hullLo = min(hullLo, sIv[grp][k].start); hullHi = max(hullHi, sIv[grp][k].end); }
    // row tiles: a slot of the border scratch
    uint32_t *border = nullptr;
    bool ok = mine && qLen > 0 && tLen > 0;
    if (G == 64 && ok && qLen > ROWS) {
        uint32_t slot = 0;
        if (lane == 0) slot = atomicAdd(V.border_next, 1u);
        slot = (uint32_t) __builtin_amdgcn_readfirstlane((int) slot);
        if (slot >= V.border_slots || (uint32_t) tLen > V.border_stride) { if (lane == 0) atomicAdd(&V.flags[1], 1u); ok = false; }
        else border = V.border + (size_t) slot * V.border_stride;
    }
    int8_t *prof = sProf + (size_t) grp * 24 * ROWS;
    const int64_t qOff = inList ? (int64_t) V.q_off[qi] : 0, tOff = inList ? (int64_t) V.t_off[ti] : 0;
    int score = 0, endCol = -1, endRow = -1;
    altali_pass<G>(V, prof, sMat, sIv[grp], nIv, hullLo, hullHi, lane, qOff, 1, ok ? qLen : 0, tOff, tLen, 0, 1, ok ? tLen : 0, border, score, endCol, endRow);
    // the gate (group-uniform): the e-value from the host's table, the coverage over (0, end cell)
    uint8_t verdict = ALT_REJECTED;
    double evalue = 0.0;
    bool reverse = false;
    if (ok && score > 0) {
        if ((uint32_t) score >= V.smax || (uint32_t) qLen > V.maxLen || V.lenIdx[qLen] < 0) verdict = ALT_BEYOND_TABLE;
        else {
            evalue = V.evalTab[(size_t) V.lenIdx[qLen] * V.smax + (uint32_t) score];
            reverse = altali_gate(V.crit, evalue, endRow, endCol, qLen, tLen);
        }
    }
    int rScore = 0, rCol = -1, rRow = -1;
    altali_pass<G>(V, prof, sMat, sIv[grp], nIv, hullLo, hullHi, lane, qOff + max(endRow, 0), -1, reverse ? endRow + 1 : 0, tOff, tLen, max(endCol, 0), -1,
                   reverse ? endCol + 1 : 0, border, rScore, rCol, rRow);
    if (mine && lane == 0) {
        mk_alignment a = {};
        if (reverse) {
            if (rScore != score) atomicAdd(&V.flags[0], 1u);
            else if (altali_record(V.crit, ti, score, endRow - rRow, endRow, endCol - rCol, endCol, qLen, tLen, evalue, V.bitScore[score], a)) {
                verdict = ALT_ACCEPTED;
                const uint32_t n = V.chain_niv[chain];
                if (n < V.iv_stride) { V.chain_iv[(size_t) chain * V.iv_stride + n] = AltInterval{a.db_start, a.db_end}; V.chain_niv[chain] = n + 1u; }
            }
        }
        store_record(&V.rec[job], a);
        V.verdict[job] = verdict;
        const unsigned long long cells = (unsigned long long) qLen * (unsigned long long) tLen + (reverse ? (unsigned long long) (endRow + 1) * (unsigned long long) (endCol + 1) : 0ull);
        atomicAdd(&V.work[0], (unsigned long long) (tLen + 2 * qLen + (reverse ? endCol + 1 + 2 * (endRow + 1) : 0)) + 8ull * (unsigned long long) nIv + sizeof(mk_alignment) + 13ull);
        atomicAdd(&V.work[1], cells);
    }
}

// ---- the next round's list: count per 256 jobs, scan, emit ----
__global__ __launch_bounds__(256) void altali_count_kernel(const uint8_t *verdict, uint32_t n, uint32_t *blockCnt) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int c = __syncthreads_count(i < n && verdict[i] == ALT_ACCEPTED);
    if (threadIdx.x == 0) blockCnt[blockIdx.x] = (uint32_t) c;
}
// one workgroup: every lane sums a contiguous run of the block counts, lane 0 scans the 256 sums, every lane rewrites its run as exclusive starts
__global__ __launch_bounds__(256) void altali_scan_kernel(uint32_t *blockCnt, uint32_t nb, uint32_t *total) {
    __shared__ uint32_t sSum[256];
    const uint32_t per = (nb + 255u) / 256u, b0 = min(nb, threadIdx.x * per), b1 = min(nb, b0 + per);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += blockCnt[b];
    sSum[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int k = 0; k < 256; k++) { const uint32_t v = sSum[k]; sSum[k] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    uint32_t run = sSum[threadIdx.x];
    for (uint32_t b = b0; b < b1; b++) { const uint32_t v = blockCnt[b]; blockCnt[b] = run; run += v; }
}
__global__ __launch_bounds__(256) void altali_emit_kernel(const uint32_t *jobs, const uint8_t *verdict, uint32_t n, const uint32_t *blockStart, uint32_t *nextJobs) {
    __shared__ uint32_t sWave[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool keep = i < n && verdict[i] == ALT_ACCEPTED;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) sWave[w] = (uint32_t) __popcll(m);
    __syncthreads();
    if (keep) {
        uint32_t r = blockStart[blockIdx.x] + (uint32_t) __popcll(m & ((1ull << lane) - 1ull));
        for (int k = 0; k < w; k++) r += sWave[k];
        nextJobs[r] = jobs[i];
    }
}

}  // namespace

hipError_t launch_altali(const AltView &V, bool anyLarge, hipStream_t stream) {
    if (V.n_jobs == 0) return hipSuccess;
    hipLaunchKernelGGL(altali_kernel<8>, dim3((V.n_jobs + 7u) / 8u), dim3(64), 0, stream, V);
    if (anyLarge) hipLaunchKernelGGL(altali_kernel<64>, dim3(V.n_jobs), dim3(64), 0, stream, V);
    return hipGetLastError();
}

hipError_t launch_altali_compact(const uint32_t *jobs, const uint8_t *verdict, uint32_t n, uint32_t *blockCnt, uint32_t *nextJobs, uint32_t *total, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t nb = (n + 255u) / 256u;
    hipLaunchKernelGGL(altali_count_kernel, dim3(nb), dim3(256), 0, stream, verdict, n, blockCnt);
    hipLaunchKernelGGL(altali_scan_kernel, dim3(1), dim3(256), 0, stream, blockCnt, nb, total);
    hipLaunchKernelGGL(altali_emit_kernel, dim3(nb), dim3(256), 0, stream, jobs, verdict, n, (const uint32_t *) blockCnt, nextJobs);
    return hipGetLastError();
}

}  // namespace mk
