// metaeuk_amd/csrc/mk_trace.hip -- the backtrace stage of --alignment-mode 3 / -a on the GPU: banded affine DP with a stored direction matrix
// and the trace, one LANE per pair (mk_trace.hpp holds the code, shared with the host twin).
// Along a row F depends on H of the left neighbour and H on F, and the rolling rows of the reference live in band coordinates whose edge
// cells are reset row by row: a pair is walked by one lane exactly as the host walks it, 64 pairs per workgroup, the jobs sorted by work so
// that the lanes of a wave finish together.  Narrow groups (2 * band + 3 <= lds_width) keep the three rolling rows as per-lane LDS columns
// [k][lane] (ds_read_b32 / ds_write_b32 bank = lane % 32 whatever k a lane is at: conflict-free); wide groups keep them in global scratch
// with the same interleaving.  Directions (four bits per cell, eight cells per word) go to global scratch as [word][lane]: the lanes of a wave
// write neighbouring words.
#include "mk_trace.hpp"
#include "mk_kernels.hpp"
#include "../../include/metaeuk_amd.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>

namespace mk {

namespace {

constexpr uint64_t MK_TRACE_MAX_LEN = 1ull << 17;       // longest sequence of the library (mk_abi.cpp: MK_MAX_SEQ_LEN)

__global__ __launch_bounds__(64) void trace_kernel(TraceLaunch L) {
    __shared__ int8_t sMat[21 * 21 + 3];
    extern __shared__ int32_t sRows[];                       // 3 rows x lds_width ints x lanes (nothing when the rows are in global scratch)
    for (int k = (int) threadIdx.x; k < 441; k += 64) sMat[k] = L.mat[k];
    __syncthreads();
    const uint32_t lane = threadIdx.x, g = blockIdx.x;
    const uint64_t id = (uint64_t) g * L.lanes + lane;
    if (lane >= L.lanes || id >= L.n_jobs) return;
    const TraceJob J = L.jobs[id];
    const uint64_t width = trace_row_ints(J.band);
    Strided<int32_t> hb, eb, hc;
    if (L.lds_width == 0) {
        // the group's rows are laid out for its widest job: three blocks of (widest x lanes) ints
        const uint64_t widest = (L.row_base[g + 1] - L.row_base[g]) / (3ull * L.lanes);
        if (width > widest) { L.out[J.slot] = TraceOut{0, 0, TRACE_STALLED, 0}; return; }       // (never: the host sized them)
        int32_t *base = L.rows + L.row_base[g] + lane;
        hb = Strided<int32_t>{base, L.lanes}; eb = Strided<int32_t>{base + widest * L.lanes, L.lanes}; hc = Strided<int32_t>{base + 2 * widest * L.lanes, L.lanes};
    } else {
        const uint32_t w = L.lds_width;
        if (width > w) { L.out[J.slot] = TraceOut{0, 0, TRACE_STALLED, 0}; return; }            // (never: the host classed them)
        const uint32_t ln = L.lanes;
        hb = Strided<int32_t>{sRows + lane, ln}; eb = Strided<int32_t>{sRows + w * ln + lane, ln}; hc = Strided<int32_t>{sRows + 2 * w * ln + lane, ln};
    }
    const Strided<uint32_t> dir{L.dirs + L.dir_base[g] + lane, L.lanes};
    const uint8_t *q = L.q_res + J.q_pos, *t = L.t_res + J.t_pos;
    const int32_t max = banded_fill(sMat, q, L.q_bias8 + J.q_pos, J.qn, t, J.tn, L.gap_open, L.gap_extend, J.band, hb, eb, hc, dir);
    TraceOut o{0, 0, TRACE_MISSED, 0};
    if (max >= J.score)
        o.status = banded_trace(q, J.qn, t, J.tn, J.band, dir, L.ops + J.ops_end, L.write_ops != 0, (uint32_t) (J.qn + J.tn), &o.bt_len, &o.identities);
    L.out[J.slot] = o;
}

}  // namespace

hipError_t launch_trace(const TraceLaunch &L, hipStream_t stream) {
    if (L.n_jobs == 0) return hipSuccess;
    if (L.lds_width > (uint32_t) TRACE_LDS_WIDTH || L.lanes == 0 || L.lanes > 64 || (size_t) L.lds_width * 3 * L.lanes * sizeof(int32_t) > 60000) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned) ((L.n_jobs + L.lanes - 1) / L.lanes);
    hipLaunchKernelGGL(trace_kernel, dim3(blocks), dim3(64), (size_t) L.lds_width * 3 * L.lanes * sizeof(int32_t), stream, L);
    return hipGetLastError();
}

int trace_host(const int8_t *mat, const uint8_t *q, const int8_t *bias8, int qn, const uint8_t *t, int tn, int score, int gapOpen, int gapExtend,
               char *ops, uint32_t opsCap, TraceResult *res) {
    *res = TraceResult{0, 0, 0, TRACE_STALLED, 0};
    if (qn <= 0 || tn <= 0) return TRACE_STALLED;
    std::vector<int32_t> rows;
    std::vector<uint32_t> dirs;
    std::vector<char> back;
    for (int band = trace_first_band(qn, tn);; band *= 2) {
        const size_t w = (size_t) trace_row_ints(band);
        rows.assign(3 * w, 0);
        dirs.assign((size_t) (trace_dir_bytes(qn, band) / 4), 0);
        res->attempts++; res->band = band;
        const Strided<int32_t> hb{rows.data(), 1}, eb{rows.data() + w, 1}, hc{rows.data() + 2 * w, 1};
        const Strided<uint32_t> dir{dirs.data(), 1};
        const int32_t max = banded_fill(mat, q, bias8, qn, t, tn, gapOpen, gapExtend, band, hb, eb, hc, dir);
        if (max >= score) {
            back.assign((size_t) qn + (size_t) tn, 0);
            res->status = banded_trace(q, qn, t, tn, band, dir, back.data() + back.size(), true, (uint32_t) back.size(), &res->bt_len, &res->identities);
            if (res->status == TRACE_OK && ops) {
                if (res->bt_len > opsCap) { res->status = TRACE_LEFT_BAND; res->bt_len = res->identities = 0; }
                else std::memcpy(ops, back.data() + back.size() - res->bt_len, res->bt_len);
            }
            return res->status;
        }
        if (band >= std::max(qn, tn)) return res->status = TRACE_STALLED;
    }
}

#define TCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return MK_ERR_DEVICE; } } while (0)

int run_trace_device(const uint8_t *dQRes, const int8_t *dQBias8, const uint8_t *dTRes, const int8_t *dMat, const TracePair *pairs, size_t n,
                     int gapOpen, int gapExtend, bool keepOps, const uint64_t *opsOff, char *ops, hipStream_t stream, TraceResult *res,
                     std::string &err, trace_timed_begin_fn tb, trace_timed_end_fn te, TraceStageStats *stats) {
    if (n == 0) return MK_OK;
    if (n >= (1ull << 32)) { err = "backtrace stage: more than 2^32 pairs in one call"; return MK_ERR_UNSUPPORTED; }
    std::vector<uint32_t> pending(n);
    std::iota(pending.begin(), pending.end(), 0u);
    for (size_t p = 0; p < n; p++) {
        if (pairs[p].qn <= 0 || pairs[p].tn <= 0) { err = "backtrace stage: empty rectangle"; return MK_ERR_ARG; }
        res[p] = TraceResult{0, 0, 0, TRACE_MISSED, trace_first_band(pairs[p].qn, pairs[p].tn)};
    }
    struct Item { uint32_t pair; uint64_t dirBytes; };
    std::vector<Item> cls[TRACE_NCLASS];
    std::vector<TraceJob> jobs;
    std::vector<uint64_t> dirBase, rowBase;
    std::vector<TraceOut> outs;
    std::vector<char> opsBack;
    while (!pending.empty()) {
        for (auto &c : cls) c.clear();
        for (uint32_t p : pending) {
            // (a pair whose directions cannot be interleaved with 63 others under the slice goes the wide way, where it may run alone)
            const uint64_t w = trace_row_ints(res[p].band), db = trace_dir_bytes(pairs[p].qn, res[p].band);
            int c = 0;
            while (c < TRACE_NCLASS - 1 && !(w <= (uint64_t) trace_class_width(c) && (db + 2ull * MK_TRACE_MAX_LEN) * (uint64_t) trace_class_lanes(c) <= TRACE_SLICE_BYTES)) c++;
            cls[c].push_back(Item{p, db});
        }
        pending.clear();
        for (int c = 0; c < TRACE_NCLASS; c++) {
            const bool wide = trace_class_width(c) == 0;
            std::vector<Item> &items = cls[c];
            // lanes of a group finish together: by work, then by pair (a fixed order: the launches of a call do not depend on anything else)
            std::sort(items.begin(), items.end(), [](const Item &a, const Item &b) { return a.dirBytes != b.dirBytes ? a.dirBytes < b.dirBytes : a.pair < b.pair; });
            size_t at = 0;
            while (at < items.size()) {
                // one launch: groups of `lanes` jobs while the scratch stays under TRACE_SLICE_BYTES
                uint32_t lanes = (uint32_t) trace_class_lanes(c);
                const auto group_bytes = [&](size_t lo, size_t hi, uint32_t ln, uint64_t *dirB, uint64_t *rowI, uint64_t *opsB) {
                    uint64_t widest = 0, ob = 0;
                    for (size_t k = lo; k < hi; k++) {
                        widest = std::max(widest, trace_row_ints(res[items[k].pair].band));
                        ob += (uint64_t) pairs[items[k].pair].qn + (uint64_t) pairs[items[k].pair].tn;
                    }
                    *dirB = items[hi - 1].dirBytes * ln;            // (sorted: the last one is the largest)
                    *rowI = wide ? 3 * widest * ln : 0;
                    *opsB = keepOps ? ob : 0;
                    return *dirB + *rowI * 4 + *opsB;
                };
                {
                    uint64_t d, r, o;
                    const size_t hi = std::min(items.size(), at + lanes);
                    if (group_bytes(at, hi, lanes, &d, &r, &o) > TRACE_SLICE_BYTES) {
                        // a pair too large to interleave with 63 others: on its own, one lane, stride 1
                        if (!wide) { err = "backtrace stage: internal error (a narrow group beyond the slice)"; return MK_ERR_DEVICE; }     // (never: `fits`)
                        lanes = 1;
                        const uint64_t need = group_bytes(at, at + 1, 1, &d, &r, &o);
                        if (need > TRACE_SLICE_BYTES) {
                            char buf[256];
                            const TracePair &P = pairs[items[at].pair];
                            snprintf(buf, sizeof(buf), "backtrace of a %d x %d rectangle at band %d needs %llu bytes of direction scratch, more than the %llu of one launch",
                                     P.qn, P.tn, res[items[at].pair].band, (unsigned long long) need, (unsigned long long) TRACE_SLICE_BYTES);
                            err = buf;
                            return MK_ERR_UNSUPPORTED;
                        }
                    }
                }
                jobs.clear(); dirBase.clear(); rowBase.clear();
                uint64_t dirTotal = 0, rowTotal = 0, opsTotal = 0, used = 0;
                double cells = 0;
                const size_t first = at;
                while (at < items.size()) {
                    const size_t hi = std::min(items.size(), at + lanes);
                    uint64_t d, r, o;
                    const uint64_t gb = group_bytes(at, hi, lanes, &d, &r, &o);
                    if (!jobs.empty() && used + gb > TRACE_SLICE_BYTES) break;
                    if (jobs.empty() && gb > TRACE_SLICE_BYTES) break;               // (the next launch decides: one lane per group)
                    dirBase.push_back(dirTotal / 4); rowBase.push_back(rowTotal);
                    for (size_t k = at; k < hi; k++) {
                        const uint32_t p = items[k].pair;
                        TraceJob J;
                        J.pad = 0; J.t_pos = pairs[p].t_pos; J.q_pos = pairs[p].q_pos; J.qn = pairs[p].qn; J.tn = pairs[p].tn; J.score = pairs[p].score;
                        J.band = res[p].band; J.slot = (uint32_t) jobs.size();
                        opsTotal += keepOps ? (uint64_t) J.qn + (uint64_t) J.tn : 0;
                        J.ops_end = opsTotal;
                        jobs.push_back(J);
                        cells += (double) trace_band_cells(J.qn, J.tn, J.band);
                    }
                    dirTotal += d; rowTotal += r; used += gb;
                    at = hi;
                    if (lanes == 1) break;                                            // the large pair alone in its launch
                }
                if (jobs.empty()) { err = "backtrace stage: internal error (empty launch)"; return MK_ERR_DEVICE; }
                rowBase.push_back(rowTotal);
                const size_t nj = jobs.size(), ng = dirBase.size();
                TraceJob *dJobs = (TraceJob *) dev_scratch("trace_jobs", nj * sizeof(TraceJob));
                TraceOut *dOut = (TraceOut *) dev_scratch("trace_out", nj * sizeof(TraceOut));
                uint64_t *dBase = (uint64_t *) dev_scratch("trace_base", (2 * ng + 1) * sizeof(uint64_t));
                uint32_t *dDirs = (uint32_t *) dev_scratch("trace_dirs", std::max<uint64_t>(dirTotal, 4));
                int32_t *dRows = (int32_t *) dev_scratch("trace_rows", std::max<uint64_t>(rowTotal, 1) * sizeof(int32_t));
                char *dOps = (char *) dev_scratch("trace_ops", std::max<uint64_t>(opsTotal, 1));
                if (!dJobs || !dOut || !dBase || !dDirs || !dRows || !dOps) { err = "backtrace stage: device allocation failed"; return MK_ERR_DEVICE; }
                TCHK(hipMemcpyAsync(dJobs, jobs.data(), nj * sizeof(TraceJob), hipMemcpyHostToDevice, stream));
                TCHK(hipMemcpyAsync(dBase, dirBase.data(), ng * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
                TCHK(hipMemcpyAsync(dBase + ng, rowBase.data(), (ng + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
                TraceLaunch L;
                L.q_res = dQRes; L.q_bias8 = dQBias8; L.t_res = dTRes; L.mat = dMat;
                L.jobs = dJobs; L.out = dOut; L.n_jobs = (uint32_t) nj;
                L.lds_width = (uint32_t) trace_class_width(c); L.lanes = lanes;
                L.dir_base = dBase; L.dirs = dDirs; L.row_base = dBase + ng; L.rows = dRows;
                L.ops = dOps; L.write_ops = keepOps ? 1u : 0u;
                L.gap_open = gapOpen; L.gap_extend = gapExtend;
                static const char *const names[TRACE_NCLASS] = {"sw_trace_lds11", "sw_trace_lds23", "sw_trace_lds67", "sw_trace_lds259", "sw_trace_lds1027", "sw_trace_global"};
                const int th = tb ? tb(names[c], (double) dirTotal + (double) nj * (sizeof(TraceJob) + sizeof(TraceOut)), cells) : -1;
                TCHK(launch_trace(L, stream));
                if (te) te(th);
                outs.resize(nj);
                TCHK(hipMemcpyAsync(outs.data(), dOut, nj * sizeof(TraceOut), hipMemcpyDeviceToHost, stream));
                if (keepOps) {
                    opsBack.resize(opsTotal);
                    TCHK(hipMemcpyAsync(opsBack.data(), dOps, opsTotal, hipMemcpyDeviceToHost, stream));
                }
                TCHK(hipStreamSynchronize(stream));
                if (stats) {
                    stats->cells += cells; stats->launches++;
                    stats->jobs[c] += nj;
                }
                for (size_t k = 0; k < nj; k++) {
                    const uint32_t p = items[first + k].pair;
                    const TraceOut &o = outs[k];
                    TraceResult &R = res[p];
                    R.attempts++;
                    if (o.status == TRACE_MISSED) {
                        if (R.band >= std::max(pairs[p].qn, pairs[p].tn)) {
                            char buf[200];
                            snprintf(buf, sizeof(buf), "Alignment score and position are not consensus: pair %u (%d x %d cells, score %d) misses its score at band %d",
                                     p, pairs[p].qn, pairs[p].tn, pairs[p].score, R.band);
                            err = buf;
                            return MK_ERR_SW_MISMATCH;
                        }
                        R.band *= 2;
                        pending.push_back(p);
                        continue;
                    }
                    if (o.status != TRACE_OK && o.status != TRACE_LEFT_BAND) { err = "backtrace stage: internal error (a job beyond its rows)"; return MK_ERR_DEVICE; }
                    R.status = o.status; R.bt_len = o.bt_len; R.identities = o.identities;
                    if (o.status == TRACE_LEFT_BAND && stats) stats->leftBand++;
                    if (keepOps && o.status == TRACE_OK) {
                        if (opsOff[p] + o.bt_len > opsOff[p + 1]) { err = "backtrace stage: the operations of a pair do not fit its region"; return MK_ERR_ARG; }
                        std::memcpy(ops + opsOff[p], opsBack.data() + jobs[k].ops_end - o.bt_len, o.bt_len);
                    }
                }
            }
        }
        std::sort(pending.begin(), pending.end());
    }
    return MK_OK;
}

}  // namespace mk
