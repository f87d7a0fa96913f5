// metaeuk_amd/csrc/mk_limits.hpp -- --max-accept / --max-rejected, one restatement for the host paths (mk_align_limit_scan, the host assembly) and
// the limit-scan kernel of the alignment stage (mk_align.hip).
// Alignment::run (M/src/alignment/Alignment.cpp:343-405) walks a query's prefilter list in list order with passedNum = 0, rejected = 0 while
// passedNum < maxAccept && rejected < maxReject: a pair that fails the length test (:370-373) counts rejected++ without being scored; a scored
// pair that passes checkCriteria is kept, passedNum++ and rejected = 0; any other scored pair counts rejected++.  `rejected` is a STREAK.
// The walk is restated on runs of at most 64 pairs as two bit masks (accepted, rejected): what lane i needs to know -- the counters behind pair i
// if the walk gets there -- is a population count and a count of leading zeros, so a wave decides a run with ballots and no loop over the lanes.
// The state carries from one run to the next; the answer does not depend on where a list is cut into runs.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mk {

constexpr uint8_t VERDICT_REJECTED = 0, VERDICT_ACCEPTED = 1, VERDICT_LENGTH = 2;      // per pair: criteria failed / kept / length test failed (never scored)
constexpr uint32_t LIMIT_OPEN = 0, LIMIT_STOP_ACCEPT = 1, LIMIT_STOP_REJECT = 2;
constexpr uint32_t LIMIT_NONE = 0x7FFFFFFFu;                                            // INT_MAX, the reference's default of both flags

struct LimitState { uint32_t passed, streak, stopped; };

// 0 means "no limit" as well, so that a zero-filled mk_params keeps the unlimited behaviour
__host__ __device__ inline uint32_t limit_of(int v) { return v <= 0 ? LIMIT_NONE : (uint32_t) v; }
__host__ __device__ inline bool limits_active(int maxAccept, int maxRejected) { return limit_of(maxAccept) != LIMIT_NONE || limit_of(maxRejected) != LIMIT_NONE; }

__host__ __device__ inline uint32_t limit_popc(uint64_t x) {
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t) __popcll((unsigned long long) x);
#else
    return (uint32_t) __builtin_popcountll(x);
#endif
}
__host__ __device__ inline uint32_t limit_top_bit(uint64_t x) {      // index of the highest set bit, x != 0
#ifdef __HIP_DEVICE_COMPILE__
    return 63u - (uint32_t) __clzll((long long) x);
#else
    return 63u - (uint32_t) __builtin_clzll(x);
#endif
}
__host__ __device__ inline uint32_t limit_low_bit(uint64_t x) {      // index of the lowest set bit, x != 0
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t) __ffsll((unsigned long long) x) - 1u;
#else
    return (uint32_t) __builtin_ctzll(x);
#endif
}
__host__ __device__ inline uint64_t limit_upto(uint32_t i) { return i >= 63u ? ~0ull : ((2ull << i) - 1ull); }   // bits 0 .. i

// Would the walk stop BEHIND pair i of the run, if it gets that far?  acc / rej: the run's accepted / rejected pairs (bit = position in the run).
// passed = the carried count + the accepted pairs up to i; streak = the rejections since the last accepted pair at or below i (the carried
// streak joins when there is none).
__host__ __device__ inline bool limit_lane_stops(const LimitState &s, uint64_t acc, uint32_t i, uint32_t maxAccept, uint32_t maxRejected) {
    const uint64_t a = acc & limit_upto(i);
    const uint32_t passed = s.passed + limit_popc(a);
    const uint32_t streak = a == 0 ? s.streak + i + 1u : i - limit_top_bit(a);
    return passed >= maxAccept || streak >= maxRejected;
}

// The run's outcome from the mask of the lanes that would stop: the walk looks at the pairs up to the first of them (all n without one).
// Returns how many pairs it looked at; kept = the accepted ones among them; s moves behind the run.
__host__ __device__ inline uint32_t limit_finish(LimitState &s, uint64_t acc, uint32_t n, uint64_t stopMask, uint64_t &kept) {
    kept = 0;
    if (s.stopped != LIMIT_OPEN || n == 0) return 0;
    const uint32_t looked = stopMask ? limit_low_bit(stopMask) + 1u : n;
    kept = acc & limit_upto(looked - 1u);
    s.passed += limit_popc(kept);
    s.streak = kept == 0 ? s.streak + looked : looked - 1u - limit_top_bit(kept);
    if (stopMask) s.stopped = ((acc >> (looked - 1u)) & 1ull) ? LIMIT_STOP_ACCEPT : LIMIT_STOP_REJECT;
    return looked;
}

// host form: the next n pairs of one query's list (any n: taken 64 at a time).  keep[k] = 1 for the accepted pairs the reference keeps (may be null).
inline uint64_t limit_step(LimitState &s, const uint8_t *verdicts, uint64_t n, uint32_t maxAccept, uint32_t maxRejected, uint8_t *keep) {
    uint64_t lookedAll = 0;
    for (uint64_t b = 0; b < n; b += 64) {
        const uint32_t m = (uint32_t) (n - b < 64 ? n - b : 64);
        uint64_t acc = 0, stop = 0, kept;
        for (uint32_t i = 0; i < m; i++) if (verdicts[b + i] == VERDICT_ACCEPTED) acc |= 1ull << i;
        if (s.stopped == LIMIT_OPEN)
            for (uint32_t i = 0; i < m; i++) if (limit_lane_stops(s, acc, i, maxAccept, maxRejected)) stop |= 1ull << i;
        lookedAll += limit_finish(s, acc, m, stop, kept);
        if (keep) for (uint32_t i = 0; i < m; i++) keep[b + i] = (uint8_t) ((kept >> i) & 1ull);
    }
    return lookedAll;
}

}  // namespace mk
