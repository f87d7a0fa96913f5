"""--max-accept / --max-rejected without a GPU: the host twin of the limit scan (mk_align_limit_scan, metaeuk_amd/csrc/mk_limits.hpp) against a
brute-force loop that restates Alignment.cpp:343-397, fed whole and in runs with the carried state; against the records the REAL `metaeuk align`
kept on the recorded prefilter lists (tests/golden/make_align_limit_golden.sh); the two new mk_params fields and their argument checks."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_MAX = 2 ** 31 - 1
F = np.float32


@pytest.fixture(scope="module")
def api():
    from metaeuk_amd import api
    return api


def _text(name):
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        return f.read()


def _lines(name):
    return _text(name).split("\n")[:-1]


def _blocks(text):
    """'>key' blocks -> {key: [lines]}"""
    out, cur = {}, None
    for ln in text.splitlines():
        if ln.startswith(">"):
            cur = out.setdefault(int(ln[1:]), [])
        else:
            cur.append(ln)
    return out


def walk(verdicts, max_accept, max_rejected, state=None):
    """the reference's loop on one list (1 = accepted, 0 = rejected, 2 = failed the length test) -> (keep flags, pairs looked at, state)"""
    lim_a = INT_MAX if max_accept == 0 else max_accept
    lim_r = INT_MAX if max_rejected == 0 else max_rejected
    passed, streak, stopped = state or (0, 0, 0)
    keep, looked = [0] * len(verdicts), 0
    for k, v in enumerate(verdicts):
        if stopped or not (passed < lim_a and streak < lim_r):
            break
        looked += 1
        if v == 1:
            keep[k] = 1; passed += 1; streak = 0
        else:
            streak += 1
        if passed >= lim_a:
            stopped = 1
        elif streak >= lim_r:
            stopped = 2
    return keep, looked, (passed, streak, stopped)


def _cases(seed=20261021):
    rs = np.random.RandomState(seed)
    lists = []
    for n in (0, 1, 63, 64, 65, 300):
        lists += [np.ones(n, np.uint8), np.zeros(n, np.uint8), (np.arange(n) % 2).astype(np.uint8), ((np.arange(n) + 1) % 2).astype(np.uint8),
                  np.full(n, 2, np.uint8)]
    for _ in range(3000):
        n = int(rs.choice([0, 1, 2, 5, 17, 63, 64, 65, 100, 128, 129, 300]))
        p_acc = rs.choice([0.02, 0.1, 0.5, 0.9])
        v = (rs.random_sample(n) < p_acc).astype(np.uint8)
        v[(v == 0) & (rs.random_sample(n) < 0.2)] = 2
        lists.append(v)
    return lists, rs


LIMITS = [(a, r) for a in (1, 2, 5, INT_MAX, 0) for r in (1, 2, 5, INT_MAX, 0)] + [(70, 70), (64, INT_MAX), (INT_MAX, 64), (INT_MAX, 65)]


def _flat(lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v in lists])
    return (np.concatenate(lists).astype(np.uint8) if len(lists) else np.zeros(0, np.uint8)), off


def test_twin_equals_the_brute_force_loop(api):
    lists, _ = _cases()
    flat, off = _flat(lists)
    for a, r in LIMITS:
        keep, looked = api.align_limit_scan(flat, off, a, r)
        for i, v in enumerate(lists):
            wk, wl, _ = walk(v.tolist(), a, r)
            assert keep[int(off[i]):int(off[i + 1])].tolist() == wk and int(looked[i]) == wl, (a, r, i, v.tolist())
    # without a limit everything accepted is kept and every pair is looked at
    keep, looked = api.align_limit_scan(flat, off, INT_MAX, 0)
    assert np.array_equal(keep, (flat == 1).astype(np.uint8)) and np.array_equal(looked, np.diff(off).astype(np.uint32))


def test_the_answer_does_not_depend_on_the_runs(api):
    lists, rs = _cases(7)
    flat, off = _flat(lists)
    n = len(lists)
    for a, r in LIMITS[::2]:
        whole_keep, whole_looked = api.align_limit_scan(flat, off, a, r)
        state = np.zeros((n, 3), dtype=np.uint32)
        pos = np.zeros(n, dtype=np.int64)
        keep = np.zeros(len(flat), dtype=np.uint8)
        looked = np.zeros(n, dtype=np.int64)
        lens = np.diff(off).astype(np.int64)
        while (pos < lens).any():
            take = np.minimum(lens - pos, rs.randint(0, 70, n))
            roff = np.zeros(n + 1, dtype=np.uint64)
            roff[1:] = np.cumsum(take)
            run = np.concatenate([flat[int(off[i]) + pos[i]:int(off[i]) + pos[i] + take[i]] for i in range(n)]) if take.sum() else np.zeros(0, np.uint8)
            k, l = api.align_limit_scan(run, roff, a, r, state=state)
            for i in np.nonzero(take)[0]:
                keep[int(off[i]) + pos[i]:int(off[i]) + pos[i] + take[i]] = k[int(roff[i]):int(roff[i + 1])]
            looked += l
            pos += take
        assert np.array_equal(keep, whole_keep) and np.array_equal(looked, whole_looked.astype(np.int64)), (a, r)
        for i in range(0, n, 97):                               # ... and the carried state is the loop's
            assert tuple(int(x) for x in state[i]) == walk(lists[i].tolist(), a, r)[2], (a, r, i)


# ---- the real process's lists --------------------------------------------------------------------------------------------------------
def can_be_covered_mode5(thr, q_len, t_len):
    a, b = F(q_len), F(t_len)
    return min(a, b) / max(a, b) >= F(thr)


CASES = {                     # name: (max_accept, max_rejected, unlimited golden, limited golden, -c of --cov-mode 5)
    "A": (1, INT_MAX, "e2e_process_aln.txt.gz", "e2e_limit_aln_A.txt.gz", 0.0),
    "B": (INT_MAX, 1, "e2e_process_aln.txt.gz", "e2e_limit_aln_B.txt.gz", 0.0),
    "C": (1, 2, "e2e_limit_aln_C_unlimited.txt.gz", "e2e_limit_aln_C.txt.gz", 0.0),
    "D": (INT_MAX, 1, "e2e_limit_aln_D_unlimited.txt.gz", "e2e_limit_aln_D.txt.gz", 0.2),
}


def recorded_verdicts(case):
    """-> (lists {query: [target keys]}, verdict arrays in list order, accepted lines {query: {target: line}})"""
    _, _, unl, _, thr = CASES[case]
    pref = _blocks(_text("e2e_process_pref.txt.gz"))
    acc = {q: {int(ln.split("\t")[0]): ln for ln in v} for q, v in _blocks(_text(unl)).items()}
    frags = [l.rsplit("\t", 1)[1] for l in _lines("e2e_process_orfs.txt.gz")]
    targets = _lines("e2e_targets.txt.gz")
    lists, verdicts = {}, {}
    for q, v in pref.items():
        lists[q] = [int(ln.split("\t")[0]) for ln in v]
        verdicts[q] = np.array([2 if thr > 0 and not can_be_covered_mode5(thr, len(frags[q]), len(targets[t])) else (1 if t in acc.get(q, {}) else 0)
                                for t in lists[q]], dtype=np.uint8)
    return lists, verdicts, acc


@pytest.mark.parametrize("case", sorted(CASES))
def test_twin_on_the_recorded_lists_keeps_what_the_real_process_kept(api, case):
    a, r, unl, lim, thr = CASES[case]
    lists, verdicts, acc = recorded_verdicts(case)
    keys = sorted(lists)
    flat, off = _flat([verdicts[q] for q in keys])
    assert len(flat) == 4777
    keep, looked = api.align_limit_scan(flat, off, a, r)
    want = _blocks(_text(lim))
    assert _text(lim) != _text(unl)
    n_changed = 0
    for i, q in enumerate(keys):
        kept = [acc[q][t] for t, k in zip(lists[q], keep[int(off[i]):int(off[i + 1])]) if k]
        assert sorted(kept) == sorted(want.get(q, [])), (case, q)
        n_changed += len(kept) != len(acc.get(q, {}))
    assert n_changed >= 20
    if case == "A":
        assert int(looked.sum()) == 1742                          # tests/golden/PROVENANCE_align_limits.txt
    if case == "C":
        assert int(looked.sum()) == 1881
    if case == "D":                                               # length-test rejections are seen at their list positions
        assert int((flat == 2).sum()) > 100 and int(looked.sum()) == 4122


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_params_layout_and_defaults(api):
    P = api.Params
    names = [f[0] for f in P._fields_]
    k = names.index("seq_id_thr")
    assert names[k + 1:k + 4] == ["max_accept", "max_rejected", "pad_"] and names[k + 4] == "alignment_mode"
    assert P.max_accept.offset == P.seq_id_thr.offset + 4 and P.max_rejected.offset == P.seq_id_thr.offset + 8
    assert C.sizeof(P) == api.lib().mk_debug_params_size() and C.sizeof(P) % 8 == 0
    p = api.default_params()
    assert (p.max_accept, p.max_rejected) == (INT_MAX, INT_MAX)


def test_negative_limits_are_refused(api):
    for kw in (dict(max_accept=-1), dict(max_rejected=-5)):
        p = api.default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        with pytest.raises(api.MkError, match="error -1") as e:
            api.result_filter(p, 50, 300)
        assert "--max-" in str(e.value)
    p = api.default_params()
    p.max_accept, p.max_rejected = 0, 3                           # 0 = no limit
    assert api.result_filter(p, 50, 300)
    v, off = np.array([1, 0], np.uint8), np.array([0, 2], np.uint64)
    with pytest.raises(api.MkError, match="error -1"):
        api.align_limit_scan(v, off, -1, 1)
    with pytest.raises(api.MkError, match="error -1"):
        api.align_limit_scan(v, off, 1, -1)
