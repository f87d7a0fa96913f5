// metaeuk_amd/csrc/mk_ungapped.hip -- the kernels of the exhaustive gapless prefilter (the rule: mk_ungapped.hpp; the design: DESIGN.md 4.1).
// Score kernel.  A gapless DP hands nothing from row to row except along a diagonal, so a lane OWNS C = UNG_DIAGS consecutive diagonals of one
// target and walks the query's rows; its C states stay in registers for the whole pair and nothing crosses a lane before the pair's last step.
// At row i diagonal d sits on column d + i: the lane keeps a window of 2 C - 1 target residues, already turned into LDS byte offsets
// (image base + row block + residue * 8), slides it by C per block of C rows, and the C rows of a block are unrolled so that every register
// index and every row offset (the immediate of the LDS read) is static.  G lanes (8, or the whole wave for long targets) sweep the L + Lq - 1
// diagonals of one target G * C at a time; the groups of a workgroup take neighbours of the length-sorted target order and finish together.
// The query is the wave-uniform side: all lanes of a workgroup walk the same rows, and UNG_PACK = 4 queries of neighbouring length share one
// lookup -- the image is [row][32 residue codes][4 queries] int16, 256 B per row, one 8-byte LDS read per four cells, then three packed int16
// operations per two cells (saturating add, max with 0, running max: the commuted form of mk_ungapped.hpp; the cap is applied once per pair).
// The image holds UNG_ROW_TILE rows; longer queries are walked tile by tile with the states kept in registers.  Code 31 is the pad line
// (-32768 for every query: it clears the state), the line a window position outside [0, L) points at -- such a position is never taken from
// memory: only aligned dwords that overlap the target are loaded, and every byte outside [0, L) is replaced before use.
// Selection kernel: one workgroup per query.  A radix select over the 40-bit key (255 - score, rank of the DB key) finds the key of the
// max_seqs-th hit in at most five histogram passes (the first over the score bytes alone), one more pass emits everything up to it, and the
// at most max_seqs keys are sorted with the bitonic network of mk_segsort.hpp.  Candidates kept from earlier target chunks enter every pass as
// further items, so a database wider than the score array is selected chunk by chunk with the same kernel.
#include "mk_ungapped.hpp"
#include "mk_kernels.hpp"
#include "mk_segsort.hpp"

namespace mk {
namespace {

constexpr int C = UNG_DIAGS, TILE = UNG_ROW_TILE, ROW_BYTES = 32 * UNG_PACK * 2, BLOCK_BYTES = C * ROW_BYTES;
static_assert(UNG_PACK == 4 && ROW_BYTES == 256, "one 8-byte LDS read feeds four queries");
static_assert(C == 8, "a row block brings eight new residues: two dwords");
static_assert(TILE % C == 0, "a tile is a whole number of row blocks");

typedef short v2s __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2s as_v2s(uint32_t x) { return __builtin_bit_cast(v2s, x); }
__device__ __forceinline__ uint32_t as_u32(v2s x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ v2s vmax(v2s a, v2s b) { return __builtin_elementwise_max(a, b); }
// U' = max(0, U + p), two queries at once
__device__ __forceinline__ v2s cell2(v2s s, uint32_t p) { return vmax(__builtin_elementwise_add_sat(s, as_v2s(p)), (v2s) (short) 0); }

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t v) { return (uint32_t) __builtin_amdgcn_update_dpp((int) v, (int) v, CTRL, 0xF, 0xF, false); }
// the maximum of the packed halves over the G lanes of a group, in every lane of it
template <int G>
__device__ __forceinline__ uint32_t group_max(uint32_t v) {
    v = as_u32(vmax(as_v2s(v), as_v2s(dpp<0xB1>(v))));           // quad_perm [1, 0, 3, 2]
    v = as_u32(vmax(as_v2s(v), as_v2s(dpp<0x4E>(v))));           // quad_perm [2, 3, 0, 1]
    v = as_u32(vmax(as_v2s(v), as_v2s(dpp<0x141>(v))));          // row_half_mirror
    if constexpr (G == 64) {
        v = as_u32(vmax(as_v2s(v), as_v2s(dpp<0x140>(v))));      // row_mirror
        v = as_u32(vmax(as_v2s(v), as_v2s((uint32_t) __shfl_xor((int) v, 16))));
        v = as_u32(vmax(as_v2s(v), as_v2s((uint32_t) __shfl_xor((int) v, 32))));
    }
    return v;
}

// one target as a lane sees it: aligned dwords from `words`, the target's first residue `r0` bytes into them
struct TargetWin { const uint32_t *words; int r0; uint32_t len; };
// the residues at target positions p .. p + 7 (p may lie in front of or behind the target) as two dwords.  Only aligned dwords that overlap
// [0, len) are loaded; what the others would hold is never used
__device__ __forceinline__ void fetch8(const TargetWin &T, int p, uint32_t &lo, uint32_t &hi) {
    const int x = T.r0 + p, base = x & ~3, first = T.r0, end = T.r0 + (int) T.len;
    uint32_t d[3];
#pragma unroll
    for (int m = 0; m < 3; m++) {
        const int b = base + 4 * m;
        d[m] = (b + 3 >= first && b < end) ? T.words[b >> 2] : 0u;
    }
    const uint32_t sh = (uint32_t) (x & 3);
    lo = __builtin_amdgcn_alignbyte(d[1], d[0], sh);
    hi = __builtin_amdgcn_alignbyte(d[2], d[1], sh);
}
// the LDS byte offsets of those eight residues for the row block at `rowOff`; a position outside the target points at the pad line
// (precondition of the entry point: residue codes 0 .. 20.  The mask keeps ANY byte inside the image's 32 lines, so a stray code cannot leave LDS;
// it is then read modulo 32, not clamped to X as the host twin does)
__device__ __forceinline__ void place8(uint32_t *w, uint32_t lo, uint32_t hi, int p, uint32_t len, uint32_t rowOff) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t word = j < 4 ? lo : hi;
        const uint32_t code8 = j & 3 ? (word >> (8 * (j & 3) - 3)) & 0xF8u : (word << 3) & 0xF8u;      // (residue code & 31) * 8
        w[j] = ((uint32_t) (p + j) < len ? code8 : (uint32_t) UNG_PAD_CODE * 8u) + rowOff;
    }
}

template <int G>
__global__ __launch_bounds__(256) void ungapped_scores_kernel(UngappedView V, uint32_t a, uint32_t b) {
    constexpr uint32_t GROUPS = 256 / G;
    __shared__ uint2 sImg[TILE * 32];
    __shared__ int8_t sMat[21 * 32];
    __shared__ uint32_t sMaxSweeps;
    __shared__ unsigned long long sWork[2];
    const uint32_t tid = threadIdx.x, sub = tid % G, grp = tid / G;
    for (uint32_t k = tid; k < 21 * 32; k += 256) sMat[k] = (k & 31) < 21 ? V.mat[(k >> 5) * 21 + (k & 31)] : (int8_t) 0;
    if (tid == 0) sMaxSweeps = 0;
    if (tid < 2) sWork[tid] = 0;

    // the four queries of this group (workgroup-uniform); an absent one has no rows
    uint64_t qOff[UNG_PACK]; uint32_t qLen[UNG_PACK]; int qBias[UNG_PACK];
    uint32_t lqMax = 0;
#pragma unroll
    for (int h = 0; h < UNG_PACK; h++) {
        const uint32_t row = blockIdx.y * UNG_PACK + h;
        qOff[h] = 0; qLen[h] = 0; qBias[h] = 0;
        if (row < V.nq) {
            const uint32_t qi = V.q_order[V.q0 + row];
            qOff[h] = V.q_off[qi]; qLen[h] = (uint32_t) (V.q_off[qi + 1] - qOff[h]); qBias[h] = 255 - (int) V.q_cap[qi];
        }
        lqMax = max(lqMax, qLen[h]);
    }

    // this lane group's target
    const uint32_t pos = a + blockIdx.x * GROUPS + grp;
    const bool valid = pos < b;
    uint32_t tIdx = 0, tLen = 0; uint64_t tOff = 0;
    if (valid) { tIdx = V.t_order[V.s0 + pos]; tOff = V.t_off[tIdx]; tLen = (uint32_t) (V.t_off[tIdx + 1] - tOff); }
    TargetWin T;
    T.words = (const uint32_t *) (V.t_res + (tOff & ~(uint64_t) 3)); T.r0 = (int) (tOff & 3); T.len = tLen;
    const uint32_t nDiag = (tLen > 0 && lqMax > 0) ? tLen + lqMax - 1 : 0;
    const uint32_t nSweeps = (nDiag + G * C - 1) / (G * C);
    __syncthreads();
    if (sub == 0 && nSweeps) atomicMax(&sMaxSweeps, nSweeps);
    __syncthreads();
    const uint32_t maxSweeps = sMaxSweeps;
    const uint32_t nTiles = (lqMax + TILE - 1) / TILE;

    v2s mLo = (v2s) (short) 0, mHi = (v2s) (short) 0;
    for (uint32_t s = 0; s < maxSweeps; s++) {
        const bool act = s < nSweeps;
        v2s sLo[C], sHi[C];
#pragma unroll
        for (int k = 0; k < C; k++) { sLo[k] = (v2s) (short) 0; sHi[k] = (v2s) (short) 0; }
        // diagonal d meets row i on column d + i; this lane's first diagonal, and the window in front of row block 0: columns d0 - 1 .. d0 + 6
        // in the slots 7 .. 14, one block stride below the image so that the first slide lands them on row block 0
        int p = (int) ((s * G + sub) * C) - (int) (lqMax - 1) - 1;
        uint32_t w[2 * C - 1], lo = 0, hi = 0, rowOff = 0u - (uint32_t) BLOCK_BYTES;
        if (act) {
            fetch8(T, p, lo, hi);
            place8(w + C - 1, lo, hi, p, tLen, rowOff);
            p += C;
            fetch8(T, p, lo, hi);
        }
        for (uint32_t tile = 0; tile < nTiles; tile++) {
            const uint32_t row0 = tile * TILE, rows = min((uint32_t) TILE, lqMax - row0), nBlocks = (rows + C - 1) / C;
            if (nTiles > 1 || s == 0) {
                // the image of the tile: [row][residue code][query] = what the cell adds (mk_ungapped.hpp: ungapped_cell); 0 behind a query's end
                for (uint32_t e = tid; e < nBlocks * C * 32; e += 256) {
                    const uint32_t r = row0 + (e >> 5), code = e & 31;
                    int v[UNG_PACK];
#pragma unroll
                    for (int h = 0; h < UNG_PACK; h++) {
                        v[h] = 0;
                        if (code == (uint32_t) UNG_PAD_CODE) v[h] = -32768;
                        else if (r < qLen[h]) {
                            const uint32_t qc = min((uint32_t) V.q_res[qOff[h] + r], 20u);
                            v[h] = ungapped_cell(sMat[min(code, 20u) * 32 + qc], V.q_bias8[qOff[h] + r], qBias[h]);
                        }
                    }
                    sImg[e] = make_uint2(((uint32_t) v[0] & 0xFFFFu) | ((uint32_t) v[1] << 16), ((uint32_t) v[2] & 0xFFFFu) | ((uint32_t) v[3] << 16));
                }
                __syncthreads();
            }
            if (act) {
                for (uint32_t blk = 0; blk < nBlocks; blk++) {
                    const uint32_t newOff = blk * BLOCK_BYTES, delta = newOff - rowOff;
                    rowOff = newOff;
#pragma unroll
                    for (int j = 0; j < C - 1; j++) w[j] = w[j + C] + delta;
                    place8(w + C - 1, lo, hi, p, tLen, rowOff);
                    p += C;
                    fetch8(T, p, lo, hi);                            // the residues of the next block, a block ahead of their use
#pragma unroll
                    for (int r = 0; r < C; r++) {
#pragma unroll
                        for (int k = 0; k < C; k++) {
                            const uint2 pr = *(const uint2 *) ((const char *) sImg + w[r + k] + r * ROW_BYTES);
                            sLo[k] = cell2(sLo[k], pr.x); sHi[k] = cell2(sHi[k], pr.y);
                            mLo = vmax(mLo, sLo[k]); mHi = vmax(mHi, sHi[k]);
                        }
                    }
                }
            }
            if (nTiles > 1) __syncthreads();                         // the tile is read out before the next one overwrites it
        }
    }

    const uint32_t gLo = group_max<G>(as_u32(mLo)), gHi = group_max<G>(as_u32(mHi));
    if (valid && sub == 0) {
        unsigned long long cells = 0;
#pragma unroll
        for (int h = 0; h < UNG_PACK; h++) {
            const uint32_t row = blockIdx.y * UNG_PACK + h;
            if (row >= V.nq) continue;
            const int m = (int) (short) ((h < 2 ? gLo : gHi) >> (16 * (h & 1)));
            int score = 0;
            if (ungapped_pair_scored(V.cov_thr, V.cov_mode, qLen[h], tLen)) {
                score = min(ungapped_cap(qBias[h]), max(m, 0));
                cells += (unsigned long long) qLen[h] * tLen;
            }
            V.scores[(size_t) row * V.ns + pos] = (uint8_t) score;
        }
        atomicAdd(&sWork[0], (unsigned long long) tLen + UNG_PACK);
        atomicAdd(&sWork[1], cells);
    }
    __syncthreads();
    if (tid < 2 && sWork[tid]) atomicAdd(&V.work[tid], sWork[tid]);
}

__global__ __launch_bounds__(256) void ungapped_caps_kernel(UngappedView V, uint8_t *caps) {
    const uint32_t qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= V.n_queries) return;
    int biasMin = 0;
    for (uint64_t i = V.q_off[qi]; i < V.q_off[qi + 1]; i++) biasMin = min(biasMin, (int) V.q_bias8[i]);
    caps[qi] = (uint8_t) ungapped_cap(ungapped_bias(V.mat_min, biasMin));
}

// ---- profile queries: the transposed kernel ("Profile queries") ----
// The long side is the query here (a 300-column profile against a 38-residue fragment), so a lane owns C consecutive diagonals e = i - j and walks the
// TARGET's positions j: at step j its cells sit on the profile columns e + j .. e + j + 7 of the line of residue t[j].  The profile is the
// workgroup-uniform side: the image is [residue code][column] int16, so the eight cells of a step are 16 contiguous bytes, and because the window
// moves by one int16 per step the image is kept twice, the second copy shifted by one column -- an even step reads copy 0, an odd step copy 1, both from
// a 4-byte-aligned address (two ds_read2_b32), and no cell is shifted in registers.  A lane group of PG lanes covers a band of PG * C diagonals of one
// target; the PGROUPS groups of a workgroup share the band's image and take `passes` targets each per band, neighbours of the length order, so the image
// of a band is written once for PGROUPS * passes targets.  The bands of all targets of a workgroup start at diagonal -(longest target - 1): a shorter
// target only finds pad columns on the diagonals in front of its own first one.  Line 21 is the pad line (a step behind the target's end) and the
// columns outside [0, Lp) hold -32768 on every line: the clamped add clears the state there.  Targets longer than PTILE steps are walked window by
// window (the states stay in registers, the window is written again per band and tile) with one target per group.
constexpr int PG = UNG_PROF_GROUP, PGROUPS = 256 / PG, PBAND = UNG_PROF_BAND, PTILE = UNG_PROF_TILE, PCOLS = PBAND + PTILE;
constexpr int PLINES = 22, PPAD_LINE = 21, PLINE_BYTES = PCOLS * 2, PCOPY_DW = PLINES * PCOLS / 2, PCOPY_BYTES = PCOPY_DW * 4;
static_assert(PG == 16, "a lane group is one DPP row");
static_assert(PTILE % C == 0 && PBAND % C == 0 && 2 * PCOPY_BYTES <= 65536, "whole step blocks; two copies of the window within LDS");

__device__ __forceinline__ void workgroup_sync_lds() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// what the image holds for (line, column) of the profile at `aln`
__device__ __forceinline__ uint32_t profile_cell(const int8_t *aln, int lp, int line, int col) {
    if (line == PPAD_LINE || col < 0 || col >= lp) return 0x8000u;
    return (uint32_t) ungapped_profile_score(aln + (size_t) col * 32, line) & 0xFFFFu;
}

__global__ __launch_bounds__(256) void ungapped_profile_scores_kernel(UngappedView V, uint32_t a, uint32_t b, uint32_t passes) {
    __shared__ uint32_t sImg[2 * PCOPY_DW];
    __shared__ uint16_t sBest[UNG_PROF_MAX_PASSES * PGROUPS];
    __shared__ unsigned long long sWork[2];
    const uint32_t tid = threadIdx.x, sub = tid % PG, grp = tid / PG;
    const uint32_t row = blockIdx.y, pi = V.q_order[V.q0 + row];
    const uint64_t pOff = V.q_off[pi];
    const int lp = (int) (V.q_off[pi + 1] - pOff);
    const int8_t *aln = V.p_aln + pOff * 32;
    // this workgroup's targets: `passes` per lane group, neighbours of the length order; the longest is the last
    const uint32_t run0 = a + blockIdx.x * PGROUPS * passes, runEnd = min(b, run0 + PGROUPS * passes);
    int maxLt = 0;
    { const uint32_t tl = V.t_order[V.s0 + runEnd - 1]; maxLt = (int) (V.t_off[tl + 1] - V.t_off[tl]); }
    for (uint32_t k = tid; k < passes * PGROUPS; k += 256) sBest[k] = 0;
    if (tid < 2) sWork[tid] = 0;
    workgroup_sync_lds();
    const int nBands = (lp > 0 && maxLt > 0) ? (lp + maxLt - 1 + PBAND - 1) / PBAND : 0, nTiles = (maxLt + PTILE - 1) / PTILE;

    for (int band = 0; band < nBands; band++) {
        const int e0 = -(maxLt - 1) + band * PBAND;               // the band's first diagonal; this lane's: e0 + sub * C
        for (uint32_t pass = 0; pass < passes; pass++) {
            const uint32_t pos = run0 + pass * PGROUPS + grp;
            uint32_t tLen = 0; uint64_t tOff = 0;
            if (pos < runEnd) { const uint32_t ti = V.t_order[V.s0 + pos]; tOff = V.t_off[ti]; tLen = (uint32_t) (V.t_off[ti + 1] - tOff); }
            TargetWin T;
            T.words = (const uint32_t *) (V.t_res + (tOff & ~(uint64_t) 3)); T.r0 = (int) (tOff & 3); T.len = tLen;
            v2s st[C / 2], m0 = (v2s) (short) 0, m1 = (v2s) (short) 0;
#pragma unroll
            for (int k = 0; k < C / 2; k++) st[k] = (v2s) (short) 0;
            uint32_t lo = 0, hi = 0;
            fetch8(T, 0, lo, hi);
            for (int tile = 0; tile < nTiles; tile++) {
                const int j0 = tile * PTILE, nBlocks = (min(PTILE, maxLt - j0) + C - 1) / C;
                if (pass == 0 || nTiles > 1) {
                    // the window of (band, tile): slot s of copy 0 is column e0 + j0 + s, of copy 1 column e0 + j0 + s + 1
                    for (uint32_t e = tid; e < (uint32_t) PCOPY_DW; e += 256) {
                        const int line = (int) (e / (PCOLS / 2)), col = e0 + j0 + 2 * (int) (e % (PCOLS / 2));
                        const uint32_t v0 = profile_cell(aln, lp, line, col), v1 = profile_cell(aln, lp, line, col + 1), v2 = profile_cell(aln, lp, line, col + 2);
                        sImg[e] = v0 | (v1 << 16);
                        sImg[PCOPY_DW + e] = v1 | (v2 << 16);
                    }
                    workgroup_sync_lds();
                }
                for (int blk = 0; blk < nBlocks; blk++) {
                    const uint32_t cl = lo, ch = hi, j = (uint32_t) (j0 + blk * C);
                    fetch8(T, (int) j + C, lo, hi);                    // the residues of the next block, a block ahead of their use
                    const uint32_t base = (sub + (uint32_t) blk) * (C * 2);
#pragma unroll
                    for (int r = 0; r < C; r++) {
                        const uint32_t code = ((r < 4 ? cl : ch) >> (8 * (r & 3))) & 0xFFu;
                        const uint32_t line = j + r < tLen ? min(code, 20u) : (uint32_t) PPAD_LINE;
                        const uint32_t *p = (const uint32_t *) ((const char *) sImg + line * PLINE_BYTES + base + (r & 1) * PCOPY_BYTES + (r & ~1) * 2);
#pragma unroll
                        for (int k = 0; k < C / 2; k++) st[k] = cell2(st[k], p[k]);
                        m0 = vmax(m0, vmax(st[0], st[1])); m1 = vmax(m1, vmax(st[2], st[3]));
                    }
                }
                if (nTiles > 1) workgroup_sync_lds();                  // the window is read out before the next one overwrites it
            }
            // the maximum of this (band, target) over the group's lanes; its first lane keeps the target's maximum over the bands
            uint32_t g = as_u32(vmax(m0, m1));
            g = as_u32(vmax(as_v2s(g), as_v2s(dpp<0xB1>(g))));         // quad_perm [1, 0, 3, 2]
            g = as_u32(vmax(as_v2s(g), as_v2s(dpp<0x4E>(g))));         // quad_perm [2, 3, 0, 1]
            g = as_u32(vmax(as_v2s(g), as_v2s(dpp<0x141>(g))));        // row_half_mirror
            g = as_u32(vmax(as_v2s(g), as_v2s(dpp<0x140>(g))));        // row_mirror
            if (sub == 0) {
                const uint32_t best = max(g & 0xFFFFu, g >> 16);       // (the halves are not negative)
                sBest[pass * PGROUPS + grp] = (uint16_t) max(best, (uint32_t) sBest[pass * PGROUPS + grp]);
            }
        }
        if (nTiles == 1) workgroup_sync_lds();                         // every pass has read the band's window
    }

    if (sub == 0) {
        unsigned long long cells = 0, bytes = 0;
        const int cap = (int) V.q_cap[pi];
        for (uint32_t pass = 0; pass < passes; pass++) {
            const uint32_t pos = run0 + pass * PGROUPS + grp;
            if (pos >= runEnd) continue;
            const uint32_t ti = V.t_order[V.s0 + pos], tLen = (uint32_t) (V.t_off[ti + 1] - V.t_off[ti]);
            int score = 0;
            if (ungapped_pair_scored(V.cov_thr, V.cov_mode, (uint32_t) lp, tLen)) {
                score = min(cap, (int) sBest[pass * PGROUPS + grp]);
                cells += (unsigned long long) lp * tLen;
            }
            V.scores[(size_t) row * V.ns + pos] = (uint8_t) score;
            bytes += (unsigned long long) tLen + 1;
        }
        atomicAdd(&sWork[0], bytes);
        atomicAdd(&sWork[1], cells);
    }
    __syncthreads();
    if (tid < 2 && sWork[tid]) atomicAdd(&V.work[tid], sWork[tid]);
}

// one wave per profile: the smallest amino-acid score of its columns
__global__ __launch_bounds__(256) void ungapped_profile_caps_kernel(UngappedView V, uint8_t *caps) {
    const uint32_t qi = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (qi >= V.n_queries) return;
    int m = 0;
    for (uint64_t c = V.q_off[qi] + lane; c < V.q_off[qi + 1]; c += 64) m = min(m, ungapped_profile_col_min(V.p_aln + c * 32));
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
    if (lane == 0) caps[qi] = (uint8_t) ungapped_cap(ungapped_bias(m, 0));
}

constexpr uint32_t SORT_TILE = 2048;
__global__ __launch_bounds__(256) void ungapped_select_kernel(UngappedView V, UngappedSelect S) {
    __shared__ uint32_t sHist[256];
    __shared__ uint64_t sK[SORT_TILE];
    __shared__ uint64_t sPrefix, sLimit;
    __shared__ uint32_t sRemaining, sDone, sCount;
    const uint32_t row = blockIdx.x, tid = threadIdx.x;
    const uint8_t *scores = V.scores + (size_t) row * V.ns;
    const uint64_t *cand = S.cand + (size_t) row * S.max_seqs;
    const uint32_t nCand = S.cand_cnt[row];
    uint64_t *out = S.tmp + (size_t) row * S.max_seqs;
    auto key_of = [&](uint32_t j) {                                   // the key of chunk target j (its score passed the threshold)
        const uint32_t idx = V.t_order[V.s0 + j];
        return ungapped_hit_key(scores[j], S.key_rank ? S.key_rank[idx] : idx);
    };
    if (tid == 0) { sPrefix = 0; sLimit = (1ull << 40) - 1; sRemaining = S.max_seqs; sDone = 0; sCount = 0; }
    __syncthreads();
    // radix select, the score byte first, then the key bytes from the top: afterwards the hits to keep are the items with key <= sLimit
    for (int level = 0; level < 5; level++) {
        if (sDone) break;
        const int shift = 32 - 8 * level;
        const uint64_t prefix = sPrefix;
        sHist[tid] = 0;
        __syncthreads();
        for (uint32_t j = tid; j < V.ns; j += 256) {
            const uint32_t sc = scores[j];
            if (!ungapped_hit_kept((int) sc, S.min_score)) continue;
            if (level == 0) { atomicAdd(&sHist[255u - sc], 1u); continue; }
            if ((uint64_t) (255u - sc) != prefix >> 32) continue;
            const uint64_t k = key_of(j);
            if ((k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sHist[(uint32_t) (k >> shift) & 255u], 1u);
        }
        for (uint32_t c = tid; c < nCand; c += 256) {
            const uint64_t k = cand[c];
            if ((k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sHist[(uint32_t) (k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t cum = 0, digit = 256;
            for (uint32_t d = 0; d < 256; d++) { if (cum + sHist[d] >= sRemaining) { digit = d; break; } cum += sHist[d]; }
            if (digit == 256) { sLimit = prefix | ((1ull << (shift + 8)) - 1); sDone = 1; }        // fewer items than room: all of them
            else {
                const uint64_t next = prefix | ((uint64_t) digit << shift);
                sRemaining -= cum; sPrefix = next;
                if (sHist[digit] == sRemaining || level == 4) { sLimit = next | ((1ull << shift) - 1); sDone = 1; }
            }
        }
        __syncthreads();
    }
    const uint64_t limit = sLimit;
    for (uint32_t j = tid; j < V.ns; j += 256) {
        const uint32_t sc = scores[j];
        if (!ungapped_hit_kept((int) sc, S.min_score) || (uint64_t) (255u - sc) > limit >> 32) continue;
        const uint64_t k = key_of(j);
        if (k <= limit) { const uint32_t at = atomicAdd(&sCount, 1u); if (at < S.max_seqs) out[at] = k; }
    }
    for (uint32_t c = tid; c < nCand; c += 256) {
        const uint64_t k = cand[c];
        if (k <= limit) { const uint32_t at = atomicAdd(&sCount, 1u); if (at < S.max_seqs) out[at] = k; }
    }
    __syncthreads();
    const uint32_t n = min(sCount, S.max_seqs);
    segsort::global_sort<256, SORT_TILE>(out, n, sK);
    __syncthreads();
    uint64_t *keep = S.cand + (size_t) row * S.max_seqs;
    for (uint32_t c = tid; c < n; c += 256) {
        const uint64_t k = out[c];
        keep[c] = k;
        if (S.last) {
            const uint32_t rank = (uint32_t) k;
            mk_hit h;
            h.seq_id = S.rank_idx ? S.rank_idx[rank] : rank; h.pref_score = 255 - (int32_t) (k >> 32); h.diagonal = 0; h.pad_ = 0;
            S.hits[(size_t) row * S.max_seqs + c] = h;
        }
    }
    if (tid == 0) { S.cand_cnt[row] = n; if (S.last) S.hit_cnt[row] = n; }
}

}  // namespace

hipError_t launch_ungapped_caps(const UngappedView &V, uint8_t *caps, hipStream_t stream) {
    if (V.n_queries == 0) return hipSuccess;
    hipLaunchKernelGGL(ungapped_caps_kernel, dim3((V.n_queries + 255) / 256), dim3(256), 0, stream, V, caps);
    return hipGetLastError();
}

hipError_t launch_ungapped_scores(const UngappedView &V, uint32_t a, uint32_t b, int group, hipStream_t stream) {
    if (b <= a || V.nq == 0) return hipSuccess;
    if (b > V.ns || (group != UNG_GROUP_SHORT && group != UNG_GROUP_LONG)) return hipErrorInvalidValue;
    const uint32_t perBlock = 256u / (uint32_t) group, qGroups = (V.nq + UNG_PACK - 1) / UNG_PACK;
    if (qGroups > 65535u) return hipErrorInvalidValue;
    const dim3 grid((b - a + perBlock - 1) / perBlock, qGroups);
    if (group == UNG_GROUP_SHORT) hipLaunchKernelGGL(ungapped_scores_kernel<UNG_GROUP_SHORT>, grid, dim3(256), 0, stream, V, a, b);
    else hipLaunchKernelGGL(ungapped_scores_kernel<UNG_GROUP_LONG>, grid, dim3(256), 0, stream, V, a, b);
    return hipGetLastError();
}

hipError_t launch_ungapped_profile_caps(const UngappedView &V, uint8_t *caps, hipStream_t stream) {
    if (V.n_queries == 0) return hipSuccess;
    hipLaunchKernelGGL(ungapped_profile_caps_kernel, dim3((V.n_queries + 3) / 4), dim3(256), 0, stream, V, caps);
    return hipGetLastError();
}

hipError_t launch_ungapped_profile_scores(const UngappedView &V, uint32_t a, uint32_t b, uint32_t passes, hipStream_t stream) {
    if (b <= a || V.nq == 0) return hipSuccess;
    if (b > V.ns || passes < 1 || passes > (uint32_t) UNG_PROF_MAX_PASSES || V.nq > 65535u || !V.p_aln) return hipErrorInvalidValue;
    const uint32_t perBlock = PGROUPS * passes;
    hipLaunchKernelGGL(ungapped_profile_scores_kernel, dim3((b - a + perBlock - 1) / perBlock, V.nq), dim3(256), 0, stream, V, a, b, passes);
    return hipGetLastError();
}

hipError_t launch_ungapped_select(const UngappedView &V, const UngappedSelect &S, hipStream_t stream) {
    if (V.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(ungapped_select_kernel, dim3(V.nq), dim3(256), 0, stream, V, S);
    return hipGetLastError();
}

}  // namespace mk
