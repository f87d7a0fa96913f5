"""The exhaustive gapless prefilter on the host: mk_ungapped_prefilter_host (the literal byte arithmetic of SmithWaterman::ungapped_alignment) against a
plain row loop over numpy int arrays with the same two saturating steps, on random pairs and the named corners."""
import ctypes

import numpy as np
import pytest

import oracle


def reference(q, t, bias8=None):
    """ssw_init's bias, then S(i, j) = subs_u8(adds_u8(S(i-1, j-1), profile byte), bias) row by row; the maximum over all cells"""
    m = oracle.aln_matrix().astype(int)
    q, t = np.asarray(q, dtype=int), np.asarray(t, dtype=int)
    cb = np.zeros(len(q), dtype=int) if bias8 is None else np.asarray(bias8, dtype=int)
    bias = abs(min(int(m.min()), 0)) + abs(min(int(cb.min()), 0))
    prev, best = np.zeros(len(t) + 1, dtype=int), 0                  # prev[j + 1] = S(i - 1, j); prev[0] = the column in front of the target
    for i in range(len(q)):
        byte = (m[t, q[i]] + cb[i] + bias) & 255                      # the int8 store of createQueryProfile, read unsigned
        cur = np.zeros(len(t) + 1, dtype=int)
        cur[1:] = np.maximum(np.minimum(prev[:-1] + byte, 255) - bias, 0)
        best, prev = max(best, int(cur.max())), cur
    return best


def saturating_pair(rs):
    """a 64-residue query that occurs verbatim inside its target, a composition bias, and the cap 255 - bias it must reach"""
    q = rs.randint(0, 20, 64).astype(np.uint8)
    t = np.concatenate([rs.randint(0, 20, 37), q, rs.randint(0, 20, 50)]).astype(np.uint8)
    cb = rs.randint(-3, 4, 64).astype(np.int8)
    return q, t, cb, 255 - abs(int(oracle.aln_matrix().min())) - abs(min(int(cb.min()), 0))


def test_twin_equals_the_row_loop_on_random_pairs():
    from metaeuk_amd import api
    rs, bad = np.random.RandomState(5), []
    for k in range(300):
        q = rs.randint(0, 21, int(rs.randint(1, 90))).astype(np.uint8)
        t = rs.randint(0, 21, int(rs.randint(0, 150))).astype(np.uint8)
        if k % 3 == 0 and len(t) > 12:                                # a mutated copy of the query's head somewhere in the target
            n = min(len(q), len(t) - 5)
            t[5:5 + n] = np.where(rs.rand(n) < 0.2, t[5:5 + n], q[:n])
        cb = rs.randint(-9, 10, len(q)).astype(np.int8) if k % 2 else None
        got, want = api.ungapped_prefilter_host(q, t, cb), reference(q, t, cb)
        if got != want:
            bad.append((k, got, want))
    assert not bad, bad[:5]


@pytest.mark.parametrize("q_len,t_len", [(1, 0), (1, 1), (1, 40), (40, 0), (40, 1), (40, 7), (7, 40)])
@pytest.mark.parametrize("bias", [False, True])
def test_corners(q_len, t_len, bias):
    from metaeuk_amd import api
    rs = np.random.RandomState(q_len * 100 + t_len)
    q = rs.randint(0, 20, q_len).astype(np.uint8)
    t = np.array(q[:t_len] if t_len <= q_len else np.concatenate([rs.randint(0, 20, t_len - q_len), q])).astype(np.uint8)
    cb = rs.randint(-5, 6, q_len).astype(np.int8) if bias else None
    assert api.ungapped_prefilter_host(q, t, cb) == reference(q, t, cb)
    assert api.ungapped_prefilter_host(q, t, cb, mat=oracle.aln_matrix()) == reference(q, t, cb)


def test_saturating_pair_scores_the_cap():
    from metaeuk_amd import api
    q, t, cb, cap = saturating_pair(np.random.RandomState(9))
    assert reference(q, t, cb) == cap and api.ungapped_prefilter_host(q, t, cb) == cap
    assert api.ungapped_prefilter_host(q, t) == 255 - abs(int(oracle.aln_matrix().min()))


def test_without_a_device_the_stage_fails_loudly():
    from metaeuk_amd import api
    try:
        import torch
        if torch.cuda.is_available():
            return
    except Exception:
        pass
    p = api.default_params()
    assert api.lib().mk_init(0) == -2
    assert api.lib().mk_ungapped_prefilter(None, None, ctypes.byref(p)) == -2 and b"mk_init" in api.lib().mk_last_error()
