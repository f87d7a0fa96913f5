// metaeuk_amd/csrc/mk_gapped.hip -- the kernels of the exhaustive gapped prefilter (the rule: mk_gapped.hpp; the design: DESIGN.md 4.1).
// Score kernel: score-only local Gotoh of every query of a chunk against every target of a chunk, one int16 per pair.  No job records, no end
// positions.  A lane group of G = 8 lanes owns one target and sweeps its columns as an anti-diagonal wavefront: at step s lane l is on column s - l
// and holds R consecutive query rows (H and E) in registers, so a tile is G x R = 32, 64 or 128 rows and every register index is static.  What crosses
// a lane boundary travels by DPP row_shr:1, three moves per step: H of the lane's last row, the running F, and the column's residue, already turned
// into the byte offset of its image line.  Lane 0 injects the residues: aligned dwords fetched three blocks of four columns ahead, shifted into place
// with v_alignbyte (target starts fall on all four bytes of a dword; a dword that does not overlap the target is never loaded).
// TWO QUERIES PER LANE: the halves of every register hold the same row of two queries of neighbouring length facing the same target, so one residue
// stream and one lookup feed both.  The image in LDS is [22 residue codes][row][2 queries] int16 (line 21 and the rows behind a query's end hold
// GAP_PAD, mk_gapped.hpp: the padding argument), built once per work item from residues, composition bias and matrix; a lane reads its R rows of the
// arriving residue as R / 4 ds_read_b128, already packed.  Per cell pair: nine packed operations (gapped_cell: add with clamp, two max, two
// unsigned subtractions with clamp and a max for each of E and F, the running maximum) -- no key, no column bookkeeping.  The maximum of the group is one
// DPP butterfly at the end of the target; saturation at 32 767 is the clamped add.
// A work item is one query pair against GAP_BLOCKS_PER_WG blocks of 32 targets, neighbours in the database's ascending-length order, so the groups of
// a wave finish together; a workgroup takes the items blockIdx.x, blockIdx.x + gridDim.x, ...  Queries beyond the largest tile run in row tiles with
// the last shape: the bottom row (H and F of both queries, 8 B per column) is parked in device memory, one strip per target in flight, written
// by the group's last lane and read by its first lane of the next tile seven steps ahead of the write to the same column.
// Profile queries (mk_gapped_prefilter_profile): targets of at most GAPP_MAX_TARGET residues go through gapped_profile_scores_kernel, which puts the
// target in the rows and walks the profile's columns (its own comment below); longer ones through this kernel's PROFILE instantiations, whose image
// builder reads the alignment profile instead of residues, composition bias and matrix.
// Barriers: the matrix is staged before any loop; every barrier stands behind the loop whose LDS traffic it orders, with its own wait.
// Selection kernel: ungapped_select_kernel's radix select and bitonic finish over int16 scores and the 47-bit key of mk_gapped.hpp, six histogram
// passes at most (two over the score alone); the threshold and the query's e-value gate are applied as the scores are read.
#include "mk_gapped.hpp"
#include "mk_kernels.hpp"
#include "mk_segsort.hpp"

namespace mk {
namespace {

constexpr int G = GAP_GROUP, GROUPS = 256 / G;
static_assert(G == 8, "the hand-over and the butterfly are written for eight lanes: half a DPP row");
static_assert(GAP_PACK == 2, "two queries in the halves of a register");

typedef short v2s __attribute__((ext_vector_type(2)));
typedef unsigned short v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2s as_v2s(uint32_t x) { return __builtin_bit_cast(v2s, x); }
__device__ __forceinline__ uint32_t as_u32(v2s x) { return __builtin_bit_cast(uint32_t, x); }
// gapped_cell's arithmetic on two int16 halves: v_pk_add_i16 clamp, v_pk_sub_u16 clamp, v_pk_max_i16
struct GapPk {
    typedef v2s V;
    static __host__ __device__ __forceinline__ v2s adds(v2s a, v2s b) { return __builtin_elementwise_add_sat(a, b); }
    static __host__ __device__ __forceinline__ v2s subs0(v2s a, v2s b) {
        return __builtin_bit_cast(v2s, __builtin_elementwise_sub_sat(__builtin_bit_cast(v2u, a), __builtin_bit_cast(v2u, b)));
    }
    static __host__ __device__ __forceinline__ v2s vmax(v2s a, v2s b) { return __builtin_elementwise_max(a, b); }
};

__device__ __forceinline__ void workgroup_sync_lds() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t old, uint32_t v) { return (uint32_t) __builtin_amdgcn_update_dpp((int) old, (int) v, CTRL, 0xF, 0xF, false); }
// the value of the lane above in the group; the group's first lane receives `top` (lane 8 of a DPP row would see the neighbouring group's last lane)
__device__ __forceinline__ uint32_t from_above(uint32_t top, uint32_t v, uint32_t sub) {
    const uint32_t x = dpp<0x111>(top, v);                         // row_shr:1
    return sub == 0 ? top : x;
}
// the maximum of the packed halves over the eight lanes of a group, in every lane of it
__device__ __forceinline__ uint32_t group_max(uint32_t v) {
    v = as_u32(GapPk::vmax(as_v2s(v), as_v2s(dpp<0xB1>(v, v))));    // quad_perm [1, 0, 3, 2]
    v = as_u32(GapPk::vmax(as_v2s(v), as_v2s(dpp<0x4E>(v, v))));    // quad_perm [2, 3, 0, 1]
    v = as_u32(GapPk::vmax(as_v2s(v), as_v2s(dpp<0x141>(v, v))));   // row_half_mirror
    return v;
}

template <int R>
struct Shape {
    static constexpr int ROWS = G * R;
    static constexpr int LINE = ROWS * 4 + 16;                      // bytes of an image line; the 16 spread the lines of different residues over the banks
    static constexpr int IMAGE = (GAP_PAD_CODE + 1) * LINE;
    static_assert(R % 4 == 0 && 256 % ROWS == 0, "a lane reads whole ds_read_b128; the image is built by 256 / ROWS threads per row");
};

// PROFILE: the queries are profiles (V.p_aln); the image is filled from their columns and everything behind it is unchanged
template <int R, bool PROFILE>
__global__ __launch_bounds__(256) void gapped_scores_kernel(GappedView V, uint32_t p0, uint32_t a, uint32_t b, uint32_t nItemsPerPair, uint32_t nItems,
                                                            uint2 *park, uint64_t parkStride) {
    typedef Shape<R> S;
    constexpr int ROWS = S::ROWS, LINE = S::LINE;
    constexpr bool TILED = R == gapped_shape_rows(GAP_SHAPES - 1);
    __shared__ __attribute__((aligned(16))) uint32_t sImg[S::IMAGE / 4];
    __shared__ int8_t sMat[21 * 21];
    __shared__ unsigned long long sWork[2];
    const uint32_t tid = threadIdx.x, sub = tid % G, grp = tid / G;
    if (!PROFILE) for (uint32_t k = tid; k < 21 * 21; k += 256) sMat[k] = V.mat[k];
    if (tid < 2) sWork[tid] = 0;
    __syncthreads();
    const v2s go2 = (v2s) (short) GAP_OPEN, ge2 = (v2s) (short) GAP_EXTEND, zero2 = (v2s) (short) 0;
    const uint32_t nTB = (b - a + GROUPS - 1) / GROUPS;
    unsigned long long bytes = 0, cells = 0;

    for (uint32_t item = blockIdx.x; item < nItems; item += gridDim.x) {
        const uint32_t pair = p0 + item / nItemsPerPair, tbg = item % nItemsPerPair;
        // the two queries of the pair (workgroup-uniform); an absent one has no rows
        uint64_t qOff[2]; uint32_t qLen[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t row = pair * 2 + h;
            qOff[h] = 0; qLen[h] = 0;
            if (row < V.nq) { const uint32_t qi = V.q_order[V.q0 + row]; qOff[h] = V.q_off[qi]; qLen[h] = (uint32_t) (V.q_off[qi + 1] - qOff[h]); }
        }
        const uint32_t lqMax = max(qLen[0], qLen[1]);
        const uint32_t nTiles = TILED ? (lqMax + ROWS - 1) / ROWS : (lqMax ? 1u : 0u);
        v2s best[GAP_BLOCKS_PER_WG];
#pragma unroll
        for (int i = 0; i < GAP_BLOCKS_PER_WG; i++) best[i] = zero2;

        for (uint32_t tile = 0; tile < nTiles; tile++) {
            const uint32_t row0 = tile * ROWS;
            {   // the image of the tile: a thread owns one row and every (256 / ROWS)-th residue code
                const uint32_t row = tid % ROWS, gi = row0 + row;
                int qc[2], cb[2]; bool real[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    real[h] = gi < qLen[h];
                    qc[h] = (!PROFILE && real[h]) ? (int) min((uint32_t) V.q_res[qOff[h] + gi], 20u) : 0;
                    cb[h] = (!PROFILE && real[h]) ? (int) V.q_bias8[qOff[h] + gi] : 0;
                }
                for (uint32_t code = tid / ROWS; code <= (uint32_t) GAP_PAD_CODE; code += 256 / ROWS) {
                    int v[2];
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        if (PROFILE) v[h] = (real[h] && code < 21u) ? gapped_profile_score(V.p_aln + (qOff[h] + gi) * 32, (int) code) : GAP_PAD;
                        else v[h] = (real[h] && code < 21u) ? gapped_cell_score(sMat[code * 21 + qc[h]], cb[h]) : GAP_PAD;
                    }
                    sImg[(code * LINE) / 4 + row] = ((uint32_t) v[0] & 0xFFFFu) | ((uint32_t) v[1] << 16);
                }
            }
            workgroup_sync_lds();
            const bool readTop = TILED && park && tile > 0, writeBottom = TILED && park && tile + 1 < nTiles;
#pragma unroll
            for (int tb = 0; tb < GAP_BLOCKS_PER_WG; tb++) {
                const uint32_t blk = tbg * GAP_BLOCKS_PER_WG + tb, pos = a + blk * GROUPS + grp;
                const bool valid = blk < nTB && pos < b;
                uint32_t tLen = 0; uint64_t tOff = 0;
                if (valid) { const uint32_t tIdx = V.t_order[V.s0 + pos]; tOff = V.t_off[tIdx]; tLen = (uint32_t) (V.t_off[tIdx + 1] - tOff); }
                // a pair that cannot be covered is not walked; the group walks when either query of the register is to be scored
                // (a row-tiled walk needs its strip of parked rows: a target longer than the strip is the caller's error and is left unscored)
                const bool walk = valid && tLen > 0 && (nTiles == 1 || (park && tLen <= parkStride)) && ((qLen[0] && gapped_pair_scored(V.cov_thr, V.cov_mode, qLen[0], tLen)) ||
                                                        (qLen[1] && gapped_pair_scored(V.cov_thr, V.cov_mode, qLen[1], tLen)));
                const uint32_t *words = (const uint32_t *) (V.t_res + (tOff & ~(uint64_t) 3));
                const uint32_t r0 = (uint32_t) (tOff & 3), nWords = walk ? (r0 + tLen + 3) / 4 : 0;
                const uint32_t steps = walk ? tLen + G - 1 : 0, nBlk = (steps + 3) / 4;
                v2s H[R], E[R], m = best[tb];
#pragma unroll
                for (int r = 0; r < R; r++) { H[r] = zero2; E[r] = zero2; }
                v2s hupPrev = zero2;
                uint32_t outH = 0, outF = 0, outRes = (uint32_t) GAP_PAD_CODE * LINE;
                uint32_t d0 = 0 < nWords ? words[0] : 0u, d1 = 1 < nWords ? words[1] : 0u, d2 = 2 < nWords ? words[2] : 0u;
                const char *mine = (const char *) sImg + sub * (R * 4);
                uint2 *parkRow = TILED && park ? park + (((size_t) blockIdx.x * GAP_BLOCKS_PER_WG + tb) * GROUPS + grp) * parkStride : nullptr;
#pragma unroll 1
                for (uint32_t kb = 0; kb < nBlk; kb++) {
                    const uint32_t cur = __builtin_amdgcn_alignbyte(d1, d0, r0);      // the residues of columns 4 kb .. 4 kb + 3
                    d0 = d1; d1 = d2; d2 = kb + 3 < nWords ? words[kb + 3] : 0u;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t s = kb * 4 + k;
                        const bool inside = s < tLen;
                        const uint32_t code = inside ? min((cur >> (8 * k)) & 0xFFu, 20u) : (uint32_t) GAP_PAD_CODE;
                        uint32_t topH = 0, topF = 0;
                        if (readTop && sub == 0 && inside) { const uint2 pr = parkRow[s]; topH = pr.x; topF = pr.y; }
                        const uint32_t inH = from_above(topH, outH, sub), res = from_above(code * LINE, outRes, sub);
                        v2s F = as_v2s(from_above(topF, outF, sub));
                        uint32_t sc[R];
#pragma unroll
                        for (int i = 0; i < R / 4; i++) {
                            const uint4 x = *(const uint4 *) (mine + res + 16 * i);
                            sc[4 * i] = x.x; sc[4 * i + 1] = x.y; sc[4 * i + 2] = x.z; sc[4 * i + 3] = x.w;
                        }
                        v2s dsave = hupPrev;
#pragma unroll
                        for (int r = 0; r < R; r++) {
                            const v2s h = gapped_cell<GapPk>(dsave, as_v2s(sc[r]), E[r], F, go2, ge2);
                            dsave = H[r]; H[r] = h;
                            m = GapPk::vmax(m, h);
                        }
                        hupPrev = as_v2s(inH);
                        outH = as_u32(H[R - 1]); outF = as_u32(F); outRes = res;
                        if (writeBottom && sub == G - 1 && s >= (uint32_t) (G - 1) && s - (G - 1) < tLen) parkRow[s - (G - 1)] = make_uint2(outH, outF);
                    }
                }
                best[tb] = m;
            }
            workgroup_sync_lds();                                     // the image is read out before the next tile or item overwrites it
        }

#pragma unroll
        for (int tb = 0; tb < GAP_BLOCKS_PER_WG; tb++) {
            const uint32_t gm = group_max(as_u32(best[tb]));
            const uint32_t blk = tbg * GAP_BLOCKS_PER_WG + tb, pos = a + blk * GROUPS + grp;
            if (!(blk < nTB && pos < b) || sub >= 2) continue;
            const uint32_t row = pair * 2 + sub;                       // lane h of the group writes query h of the register
            if (row >= V.nq) continue;
            const uint32_t tIdx = V.t_order[V.s0 + pos], tLen = (uint32_t) (V.t_off[tIdx + 1] - V.t_off[tIdx]), ql = sub ? qLen[1] : qLen[0];
            int score = 0;
            if (tLen > 0 && gapped_pair_scored(V.cov_thr, V.cov_mode, ql, tLen)) {
                score = (int) (short) (gm >> (16 * sub));
                cells += (unsigned long long) ql * tLen;
            }
            V.scores[(size_t) row * V.ns + pos] = (int16_t) score;
            bytes += 2 + (sub == 0 ? tLen : 0);
        }
    }
    if (bytes) atomicAdd(&sWork[0], bytes);
    if (cells) atomicAdd(&sWork[1], cells);
    __syncthreads();
    if (tid < 2 && sWork[tid]) atomicAdd(&V.work[tid], sWork[tid]);
}

// ---- profile queries, the target in the rows ----
// A lane group owns one target of at most G x R residues, lane l its residues l R .. l R + R - 1 as rows; the steps are the profile's columns in
// blocks of four, and at step kb lane l works on block kb - l: the block the lane above it finished one step earlier.  Inside a block a lane runs
// row-major over its R x 4 cells.  Across blocks it carries E and the H of the block's last column per row (2 R registers); inside a block F per
// column (4) and the row above's H over the block's columns plus the diagonal (5).  The bottom row's H[4] and F[4] travel to the next lane by
// row_shr:1 once per block; no residue travels: the byte offset of a row's image line is computed once per target.
// The image in LDS is [22 lines: 20 residues, X, the pad line][column][2 profiles] int16, so the four columns of a block for one residue are 16
// aligned bytes: one ds_read_b128 per row and block, packed for both profiles of the register pair.  It is a window over the columns of WB steps and
// the seven blocks of lane lag in front of them (image block i of window w = column block w WB + i - 7), refilled behind a barrier; columns in
// front of column 0 and behind a profile's end hold GAP_PAD (mk_gapped.hpp: the padding argument, transposed).  The step count depends on the
// profile pair only, so every group of a workgroup walks the same steps and the barriers stand in uniform control flow, each behind the loop
// whose LDS traffic it orders.
namespace prof {
constexpr int CB = GAPP_BLOCK, LAGB = G - 1, WB = GAPP_WINDOW / CB, IBLK = WB + LAGB, ICOLS = IBLK * CB;
constexpr int LINE = ICOLS * 4;                                    // bytes of an image line: a column is two int16
constexpr int IMAGE = (GAP_PAD_CODE + 1) * LINE;
static_assert(CB == 4 && LINE % 16 == 0, "a block of one line is one aligned ds_read_b128");
static_assert(IMAGE <= 32 * 1024, "two workgroups and more per compute unit");
}  // namespace prof

template <int R>
__global__ __launch_bounds__(256) void gapped_profile_scores_kernel(GappedView V, uint32_t a, uint32_t b, uint32_t nItemsPerPair, uint32_t nItems) {
    using namespace prof;
    __shared__ __attribute__((aligned(16))) uint32_t sImg[IMAGE / 4];
    __shared__ unsigned long long sWork[2];
    const uint32_t tid = threadIdx.x, sub = tid % G, grp = tid / G;
    if (tid < 2) sWork[tid] = 0;
    __syncthreads();
    const v2s go2 = (v2s) (short) GAP_OPEN, ge2 = (v2s) (short) GAP_EXTEND, zero2 = (v2s) (short) 0;
    const uint32_t nTB = (b - a + GROUPS - 1) / GROUPS;
    unsigned long long bytes = 0, cells = 0;

    for (uint32_t item = blockIdx.x; item < nItems; item += gridDim.x) {
        const uint32_t pair = item / nItemsPerPair, tbg = item % nItemsPerPair;
        // the two profiles of the pair (workgroup-uniform); an absent one has no columns
        uint64_t pOff[2]; uint32_t pLen[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const uint32_t row = pair * 2 + h;
            pOff[h] = 0; pLen[h] = 0;
            if (row < V.nq) { const uint32_t qi = V.q_order[V.q0 + row]; pOff[h] = V.q_off[qi]; pLen[h] = (uint32_t) (V.q_off[qi + 1] - pOff[h]); }
        }
        const uint32_t lpMax = max(pLen[0], pLen[1]);
        const uint32_t steps = lpMax ? (lpMax + CB - 1) / CB + LAGB : 0, nWin = (steps + WB - 1) / WB;

#pragma unroll 1
        for (int tb = 0; tb < GAP_BLOCKS_PER_WG; tb++) {
            const uint32_t blk = tbg * GAP_BLOCKS_PER_WG + tb, pos = a + blk * GROUPS + grp;
            const bool valid = blk < nTB && pos < b;
            uint32_t tLen = 0; uint64_t tOff = 0;
            if (valid) { const uint32_t tIdx = V.t_order[V.s0 + pos]; tOff = V.t_off[tIdx]; tLen = (uint32_t) (V.t_off[tIdx + 1] - tOff); }
            // a pair that cannot be covered is not walked; the group walks when either profile of the register is to be scored (a target beyond the
            // shape's rows is the caller's error and is left unscored)
            const bool walk = valid && tLen > 0 && tLen <= (uint32_t) (G * R) && ((pLen[0] && gapped_pair_scored(V.cov_thr, V.cov_mode, pLen[0], tLen)) ||
                                                                                  (pLen[1] && gapped_pair_scored(V.cov_thr, V.cov_mode, pLen[1], tLen)));
            // the image lines of the lane's rows: fixed for the whole walk; a row behind the target's end reads the pad line
            uint32_t line[R];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t i = sub * R + r;
                line[r] = (walk && i < tLen ? min((uint32_t) V.t_res[tOff + i], 20u) : (uint32_t) GAP_PAD_CODE) * LINE;
            }
            v2s E[R], Hl[R], m = zero2, hDiag = zero2;                  // hDiag: the bottom row of the lane above in the column in front of the block
#pragma unroll
            for (int r = 0; r < R; r++) { E[r] = zero2; Hl[r] = zero2; }
            uint32_t outH[CB] = {0, 0, 0, 0}, outF[CB] = {0, 0, 0, 0};

            for (uint32_t w = 0; w < nWin; w++) {
                if (tb == 0 || nWin > 1) {
                    // the window's image: a thread takes one column of one profile, 32 bytes of it, and writes its 22 lines
                    for (uint32_t k = tid; k < (uint32_t) ICOLS * 2; k += 256) {
                        const uint32_t ic = k >> 1, h = k & 1;
                        const int64_t col = (int64_t) w * (WB * CB) + ic - LAGB * CB;
                        const bool real = col >= 0 && col < (int64_t) pLen[h];
                        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
                        if (real) { const uint4 *src = (const uint4 *) (V.p_aln + (pOff[h] + (uint64_t) col) * 32); lo = src[0]; hi = src[1]; }
                        const uint32_t wds[5] = {lo.x, lo.y, lo.z, lo.w, hi.x};
                        int16_t *dst = (int16_t *) sImg + ic * 2 + h;
#pragma unroll
                        for (int code = 0; code <= GAP_PAD_CODE; code++) {
                            const int s = code < 20 ? (int) (int8_t) (wds[code >> 2] >> (8 * (code & 3))) : 0;      // (gapped_profile_score on the loaded bytes)
                            dst[code * (LINE / 2)] = (int16_t) (real && code < 21 ? s : GAP_PAD);
                        }
                    }
                }
                workgroup_sync_lds();
                if (walk) {
                    const uint32_t k0 = w * WB, k1 = min(steps, k0 + WB);
                    const char *mine = (const char *) sImg + (LAGB - sub) * 16;
#pragma unroll 1
                    for (uint32_t kb = k0; kb < k1; kb++) {
                        v2s up[CB + 1], F[CB];
                        up[0] = hDiag;
#pragma unroll
                        for (int c = 0; c < CB; c++) {
                            up[c + 1] = as_v2s(from_above(0u, outH[c], sub));
                            F[c] = as_v2s(from_above(0u, outF[c], sub));
                        }
                        hDiag = up[CB];
                        const char *at = mine + (kb - k0) * 16;
#pragma unroll
                        for (int r = 0; r < R; r++) {
                            const uint4 x = *(const uint4 *) (at + line[r]);
                            const uint32_t sc[CB] = {x.x, x.y, x.z, x.w};
                            v2s d = up[0], e = E[r];
                            up[0] = Hl[r];
#pragma unroll
                            for (int c = 0; c < CB; c++) {
                                const v2s h = gapped_cell<GapPk>(d, as_v2s(sc[c]), e, F[c], go2, ge2);
                                d = up[c + 1]; up[c + 1] = h;
                                m = GapPk::vmax(m, h);
                            }
                            Hl[r] = up[CB]; E[r] = e;
                        }
#pragma unroll
                        for (int c = 0; c < CB; c++) { outH[c] = as_u32(up[c + 1]); outF[c] = as_u32(F[c]); }
                    }
                }
                workgroup_sync_lds();                                 // the window is read out before the next one, target block or item overwrites it
            }

            const uint32_t gm = group_max(as_u32(m));
            if (!valid || sub >= 2) continue;
            const uint32_t row = pair * 2 + sub;                       // lane h of the group writes profile h of the register
            if (row >= V.nq) continue;
            const uint32_t pl = sub ? pLen[1] : pLen[0];
            int score = 0;
            if (walk && gapped_pair_scored(V.cov_thr, V.cov_mode, pl, tLen)) {
                score = (int) (short) (gm >> (16 * sub));
                cells += (unsigned long long) pl * tLen;
            }
            V.scores[(size_t) row * V.ns + pos] = (int16_t) score;
            bytes += 2 + (sub == 0 ? tLen : 0);
        }
    }
    if (bytes) atomicAdd(&sWork[0], bytes);
    if (cells) atomicAdd(&sWork[1], cells);
    __syncthreads();
    if (tid < 2 && sWork[tid]) atomicAdd(&V.work[tid], sWork[tid]);
}

constexpr uint32_t SORT_TILE = 2048;
constexpr int LEVELS = (GAP_KEY_BITS + 7) / 8;
__global__ __launch_bounds__(256) void gapped_select_kernel(GappedView V, GappedSelect S) {
    __shared__ uint32_t sHist[256];
    __shared__ uint64_t sK[SORT_TILE];
    __shared__ uint64_t sPrefix, sLimit;
    __shared__ uint32_t sRemaining, sDone, sCount;
    __shared__ GateEntry sGate;
    const uint32_t row = blockIdx.x, tid = threadIdx.x;
    const int16_t *scores = V.scores + (size_t) row * V.ns;
    const uint64_t *cand = S.cand + (size_t) row * S.max_seqs;
    const uint32_t nCand = S.cand_cnt[row];
    uint64_t *out = S.tmp + (size_t) row * S.max_seqs;
    auto key_of = [&](uint32_t j) {                                   // the key of chunk target j (its score passed the verdict)
        const uint32_t idx = V.t_order[V.s0 + j];
        return gapped_hit_key((uint32_t) scores[j], S.key_rank ? S.key_rank[idx] : idx);
    };
    if (tid == 0) {
        sPrefix = 0; sLimit = (1ull << (8 * LEVELS)) - 1; sRemaining = S.max_seqs; sDone = 0; sCount = 0;
        if (V.gate) { const uint32_t qi = V.q_order[V.q0 + row]; sGate = V.gate[V.q_off[qi + 1] - V.q_off[qi]]; }
    }
    __syncthreads();
    const GateEntry *gate = V.gate ? &sGate : nullptr;
    // radix select, the two score bytes first, then the rank bytes from the top: afterwards the hits to keep are the items with key <= sLimit
    for (int level = 0; level < LEVELS; level++) {
        if (sDone) break;
        const int shift = 8 * (LEVELS - 1 - level);
        const uint64_t prefix = sPrefix;
        sHist[tid] = 0;
        __syncthreads();
        for (uint32_t j = tid; j < V.ns; j += 256) {
            const int sc = scores[j];
            if (!gapped_hit_kept(sc, S.min_score, gate)) continue;
            const uint64_t hi = gapped_hit_key((uint32_t) sc, 0);
            if (level < 2) { if ((hi >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sHist[(uint32_t) (hi >> shift) & 255u], 1u); continue; }
            if (hi >> 32 != prefix >> 32) continue;
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
                if (sHist[digit] == sRemaining || level == LEVELS - 1) { sLimit = next | ((1ull << shift) - 1); sDone = 1; }
            }
        }
        __syncthreads();
    }
    const uint64_t limit = sLimit;
    for (uint32_t j = tid; j < V.ns; j += 256) {
        const int sc = scores[j];
        if (!gapped_hit_kept(sc, S.min_score, gate) || gapped_hit_key((uint32_t) sc, 0) >> 32 > limit >> 32) continue;
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
            h.seq_id = S.rank_idx ? S.rank_idx[rank] : rank; h.pref_score = GAP_SCORE_CAP - (int32_t) (k >> 32); h.diagonal = 0; h.pad_ = 0;
            S.hits[(size_t) row * S.max_seqs + c] = h;
        }
    }
    if (tid == 0) { S.cand_cnt[row] = n; if (S.last) S.hit_cnt[row] = n; }
}

template <int R>
void launch_shape(const GappedView &V, uint32_t p0, uint32_t a, uint32_t b, uint32_t perPair, uint32_t items, uint2 *park, uint64_t parkStride, uint32_t blocks,
                  hipStream_t stream) {
    if (V.p_aln) hipLaunchKernelGGL((gapped_scores_kernel<R, true>), dim3(blocks), dim3(256), 0, stream, V, p0, a, b, perPair, items, park, parkStride);
    else hipLaunchKernelGGL((gapped_scores_kernel<R, false>), dim3(blocks), dim3(256), 0, stream, V, p0, a, b, perPair, items, park, parkStride);
}

}  // namespace

hipError_t launch_gapped_scores(const GappedView &V, int shape, uint32_t p0, uint32_t p1, uint32_t a, uint32_t b, uint2 *park, uint64_t parkStride,
                                uint32_t blocks, hipStream_t stream) {
    if (b <= a || p1 <= p0) return hipSuccess;
    if (b > V.ns || 2ull * p0 >= V.nq || shape < 0 || shape >= GAP_SHAPES) return hipErrorInvalidValue;
    const uint32_t nTB = (b - a + GROUPS - 1) / GROUPS, perPair = (nTB + GAP_BLOCKS_PER_WG - 1) / GAP_BLOCKS_PER_WG;
    const uint64_t items = (uint64_t) perPair * (p1 - p0);
    if (items > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (blocks == 0 || blocks > items) blocks = (uint32_t) items;
    if (shape != GAP_SHAPES - 1) { park = nullptr; parkStride = 0; }
    switch (shape) {
        case 0: launch_shape<gapped_shape_rows(0)>(V, p0, a, b, perPair, (uint32_t) items, park, parkStride, blocks, stream); break;
        case 1: launch_shape<gapped_shape_rows(1)>(V, p0, a, b, perPair, (uint32_t) items, park, parkStride, blocks, stream); break;
        default: launch_shape<gapped_shape_rows(2)>(V, p0, a, b, perPair, (uint32_t) items, park, parkStride, blocks, stream); break;
    }
    return hipGetLastError();
}

hipError_t launch_gapped_profile_scores(const GappedView &V, int shape, uint32_t a, uint32_t b, hipStream_t stream) {
    if (b <= a || V.nq == 0) return hipSuccess;
    if (b > V.ns || !V.p_aln || shape < 0 || shape >= GAP_SHAPES) return hipErrorInvalidValue;
    const uint32_t nTB = (b - a + GROUPS - 1) / GROUPS, perPair = (nTB + GAP_BLOCKS_PER_WG - 1) / GAP_BLOCKS_PER_WG;
    const uint64_t items = (uint64_t) perPair * ((V.nq + 1) / 2);
    if (items > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t) items), block(256);
    switch (shape) {
        case 0: hipLaunchKernelGGL(gapped_profile_scores_kernel<gapped_shape_rows(0)>, grid, block, 0, stream, V, a, b, perPair, (uint32_t) items); break;
        case 1: hipLaunchKernelGGL(gapped_profile_scores_kernel<gapped_shape_rows(1)>, grid, block, 0, stream, V, a, b, perPair, (uint32_t) items); break;
        default: hipLaunchKernelGGL(gapped_profile_scores_kernel<gapped_shape_rows(2)>, grid, block, 0, stream, V, a, b, perPair, (uint32_t) items); break;
    }
    return hipGetLastError();
}

hipError_t launch_gapped_select(const GappedView &V, const GappedSelect &S, hipStream_t stream) {
    if (V.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(gapped_select_kernel, dim3(V.nq), dim3(256), 0, stream, V, S);
    return hipGetLastError();
}

}  // namespace mk
