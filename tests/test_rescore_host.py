"""rescorediagonal --rescore-mode 2 without a GPU: mk_rescore_diagonal_host (csrc/mk_rescore.hpp, prefix-sum form) against the literal loop of
DistanceCalculator.h:98-111 / :183-200 in Python integers and against the real binary's records (tests/golden/make_rescore_golden.sh)."""
import functools

import numpy as np
import pytest

import oracle
from test_backtrace_host import _blocks, _lines, _text


@functools.lru_cache(None)
def mat():
    return oracle.aln_matrix().astype(int)


def reference(q, t, d16):
    """computeUngappedAlignment + ungappedAlignmentByDiagonal + computeSubstitutionStartEndDistance -> (score, start, end, real diagonal)"""
    m, best = mat(), (0, -1, -1, 0)
    for real in [-d * 65536 + d16 for d in range(1, 2 + len(t) // 32768)] + [d * 65536 + d16 for d in range(0, 1 + len(q) // 65536)]:
        if abs(real) >= (len(q) if real >= 0 else len(t)):
            continue                                     # the real diagonal misses the rectangle
        s1, s2 = (q[real:], t) if real >= 0 else (q, t[-real:])
        max_score, max_end, max_start, score, min_pos = 0, 0, 0, 0, -1
        for pos in range(min(len(s1), len(s2))):
            score += int(m[s1[pos], s2[pos]])
            if score <= 0:
                score, min_pos = 0, pos
            if score > max_score:
                max_end, max_start, max_score = pos, min_pos + 1, score
        if max_score > best[0]:
            best = (max_score, max_start, max_end, real)
    return best


def cell(score):                                         # a (query code, target code) pair of that score
    i, j = np.argwhere(mat()[:20, :20] == score)[0]
    return int(i), int(j)


# name: (cell scores from the diagonal's first cell on, query length, target length, real diagonal)
CASES = {
    "len1": ([4], 1, 1, 0), "len2": ([4, 5], 2, 2, 0), "len3": ([4, -4, 5], 3, 3, 0), "len4": ([-1, 4, 4, -4], 4, 4, 0), "len5": ([4, 4, -4, -4, 9], 5, 5, 0),
    "one cell, query corner": ([6], 9, 7, 8), "one cell, target corner": ([6], 9, 7, -6),
    "positive diagonal": ([4, 5, -1, 6], 12, 4, 8), "negative diagonal": ([4, 5, -1, 6], 4, 12, -8),
    "two equal maxima, the first wins": ([4, 4, -4, -4, 4, 4, -1], 7, 7, 0),
    "the sum touches 0 before the maximum": ([4, -4, 5, 5, -1], 5, 5, 0),
    "two resets, the latest is the start": ([-1, 4, -4, 4, -4, 9, -1], 7, 9, -2),
    "all negative": ([-1, -2, -3, -1], 4, 4, 0),
    "maximum at position 0": ([9, -4, 4, -1], 4, 6, 0), "maximum at the last position": ([1, -1, 1, 5], 6, 4, 2),
}


def check(api, q, t, d16):
    kept, a, ids = api.rescore_diagonal_host(q, t, d16, 10 ** 7, api.default_params(), mat=mat())
    score, start, end, rd = reference(q, t, d16)
    qs, ts = (start + rd, start) if rd >= 0 else (start, start - rd)
    want_ids = sum(1 for k in range(end - start + 1) if q[qs + k] == t[ts + k]) if score > 0 else 0
    assert (a.raw_score, a.q_start, a.q_end, a.db_start, a.db_end, a.aln_len, ids) == (score, qs, qs + end - start, ts, ts + end - start, end - start + 1, want_ids)
    return score, start, end, rd


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_equals_the_sequential_loop(name):
    from metaeuk_amd import api
    cells, q_len, t_len, real = CASES[name]
    rs = np.random.RandomState(1)
    q, t = rs.randint(0, 20, q_len).astype(np.uint8), rs.randint(0, 20, t_len).astype(np.uint8)
    for k, s in enumerate(cells):
        q[max(real, 0) + k], t[max(-real, 0) + k] = cell(s)
    check(api, q, t, real & 0xFFFF)                      # ("all negative": the reference's empty LocalAlignment, start = end = -1)


def test_long_target_takes_the_best_real_diagonal_not_the_first():
    """70 000 target residues: 65436 stands for -100 (walked first: a weak match), -65636 (second: the strong one), -131172 and 65436 (both miss)"""
    from metaeuk_amd import api
    rs = np.random.RandomState(4)
    t, q = rs.randint(0, 20, 70000).astype(np.uint8), rs.randint(0, 20, 120).astype(np.uint8)
    q[5:25], q[40:100] = t[105:125], t[65636 + 40:65636 + 100]
    assert check(api, q, t, 65436)[3] == -65636


# ---- the pin to the reference: the three runs of the real binary over the e2e prefilter result: (parameters, the command's flags) --------
FIXTURES = {
    "e2e_process_rescore.txt.gz": (dict(evalue_thr=0.001), []),
    "e2e_process_rescore_a_sorted.txt.gz": (dict(evalue_thr=0.001, add_backtrace=1, sort=1), ["-a", "1", "--sort-results", "1"]),
    "e2e_process_rescore_c05_id03.txt.gz": (dict(evalue_thr=0.001, cov_thr=0.5, cov_mode=2, seq_id_thr=0.3, seq_id_mode=1),
                                            ["-c", "0.5", "--cov-mode", "2", "--min-seq-id", "0.3", "--seq-id-mode", "1", "-e", "0.001"]),
}


def fixture_params(api, flags):
    p = api.default_params()
    p.min_aln_len = 0                                    # the module's own defaults (Parameters.cpp:504-521), not predictexons'
    for k in set(flags) - {"sort"}:
        setattr(p, k, flags[k])
    return p


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_host_twin_reproduces_the_real_rescorediagonal(name):
    from metaeuk_amd import api
    flags, p = FIXTURES[name][0], fixture_params(api, FIXTURES[name][0])
    codes = lambda seqs: (lambda res, off: [res[int(off[k]):int(off[k + 1])] for k in range(len(seqs))])(*api.encode(seqs))
    frags, targets = codes([l.rsplit("\t", 1)[1] for l in _lines("e2e_process_orfs.txt.gz")]), codes(_lines("e2e_targets.txt.gz"))
    want, pref, bad = _blocks(_text(name)), _blocks(_text("e2e_process_pref.txt.gz")), []
    assert sorted(want) == sorted(pref)
    for key, hits in pref.items():
        recs = []
        for tk, _, diag in (map(int, ln.split("\t")) for ln in hits):
            kept, a, _ = api.rescore_diagonal_host(frags[key], targets[tk], diag & 0xFFFF, sum(len(t) for t in targets), p)
            a.db_key = tk
            recs += [a] if kept else []
        if flags.get("sort"):
            recs.sort(key=lambda a: (a.evalue, -a.bit_score, a.db_len, a.db_key))
        got = [(api.format_alignment_bt(a, b"M" * a.aln_len) if p.add_backtrace else api.format_alignments([a], 0, 1).encode()).decode()[:-1] for a in recs]
        if got != want[key]:
            bad.append((key, got, want[key]))
    assert not bad, (len(bad), bad[:2])
