"""mk_backtrace_profile_host (banded_sw<PROFILE_SEQ> + computerBacktrace, no GPU) against the sequence twin and an unbanded Gotoh on golden columns."""
import numpy as np
import pytest

import oracle
import sw_cases
from metaeuk_amd import api
from test_gpu_profile import _golden_inputs


def gotoh(S):
    """local alignment over the score matrix S [rows, cols], gap costs 11 / 1, unbanded -> (maximum, row, column of its first cell in row order)"""
    n, m = S.shape
    H = np.zeros((n + 1, m + 1), dtype=np.int64); E = np.full((n + 1, m + 1), -10 ** 9, dtype=np.int64); F = E.copy()
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i, j] = max(H[i - 1, j] - 11, E[i - 1, j] - 1)
            F[i, j] = max(H[i, j - 1] - 11, F[i, j - 1] - 1)
            H[i, j] = max(0, H[i - 1, j - 1] + S[i - 1, j - 1], E[i, j], F[i, j])
    return (int(H.max()),) + tuple(int(x) - 1 for x in np.argwhere(H == H.max())[0])


@pytest.mark.parametrize("label", ["G4/a", "G4/b", "G4/c", "G4/d", "G4/e"])
def test_sequence_as_profile_equals_the_sequence_twin(label):
    """a profile whose column i is mat[q_i][.] without a bias is the sequence q: the ops, identities and attempts of backtrace_host (G4/e: wider bands)"""
    cs, mat, n, most = sw_cases.group("G4"), oracle.aln_matrix(), 0, 0
    for q, t, lab in cs.pairs():
        score, qe, te, qs, ts, _ = cs.expected()[(q, t)]
        if not lab.startswith(label) or score <= 0:
            continue
        qc, tc = oracle.encode(cs.queries[q]), oracle.encode(cs.targets[t])[ts:te + 1]
        aln32 = np.zeros((len(qc), 32), dtype=np.int8)
        aln32[:, :21] = mat[qc]
        want = api.backtrace_host(mat, qc[qs:qe + 1], np.zeros(qe - qs + 1, dtype=np.int8), tc, score)
        got = api.backtrace_profile_host(aln32, qc, qs, qe - qs + 1, tc, score)
        assert want[0] is not None and got == want, cs.describe(q, t)
        n, most = n + 1, max(most, got[2])
    assert n >= 4 and (label != "G4/e" or most >= 3)


# a target from 60 consensus codes: a copy (band 1); X inside; equal spans with a 4-column and a 4-residue gap (three bands); longer; a rectangle of one cell
PLANT = {"copy": lambda c: c, "x": lambda c: c[:20] + [20] + c[21:], "gaps": lambda c: c[:15] + c[19:40] + [0, 5, 9, 12] + c[40:],
         "insert": lambda c: c[:25] + [3, 17, 8] + c[25:], "one": lambda c: c[30:31]}


@pytest.mark.parametrize("kind", sorted(PLANT))
@pytest.mark.parametrize("prof,lo", [(0, 0), (1, 7), (3, 30)])
def test_golden_columns_against_gotoh(prof, lo, kind):
    """real profile columns, q_start > 0: the ops start and end in M, consume the rectangle, re-score to the Gotoh score, count equal letters"""
    e = _golden_inputs()[1][prof]
    _, _, aln, letters = oracle.profile_arrays(e, (len(e) - 1) // 25)        # the alignment profile [cols, 21] and the query letters
    aln32 = np.concatenate([aln, np.zeros((len(aln), 11), dtype=np.int8)], axis=1)
    t = np.array(PLANT[kind](list(aln32[lo + 5:lo + 65, :20].argmax(axis=1))), dtype=np.int64)
    S = np.where(t[None, :] < 20, aln32[lo:lo + 75, np.minimum(t, 19)].astype(np.int64), 0)      # X scores 0
    best, qe, te = gotoh(S)
    back, qr, tr = gotoh(S[:qe + 1, :te + 1][::-1, ::-1])                  # the reversed pass from the end cell: the start
    qs, ts = qe - qr, te - tr
    assert back == best == gotoh(S[qs:qe + 1, ts:te + 1])[0] and qs + lo > 0 and (kind != "x" or ts < 20 < te)
    ops, ids, att = api.backtrace_profile_host(aln32, letters, lo + qs, qe - qs + 1, t[ts:te + 1], best)
    ops = ops.decode()
    assert ops[0] == ops[-1] == "M" and ops.count("M") + ops.count("I") == qe - qs + 1 and ops.count("M") + ops.count("D") == te - ts + 1
    i, j, total, same = qs, ts, 0, 0
    for k, op in enumerate(ops):
        if op == "M":
            total, same, i, j = total + int(S[i, j]), same + int(letters[lo + i] == t[j]), i + 1, j + 1
        else:
            total, i, j = total - (1 if ops[k - 1] == op else 11), i + (op == "I"), j + (op == "D")
    assert (total, same) == (best, ids)
    assert att == 1 if kind in ("copy", "x", "one") else kind != "gaps" or (att >= 3 and qe - qs == te - ts and "I" in ops and "D" in ops)
    with pytest.raises(api.MkError, match="error -4.*not consensus"):      # a score no band can reach: the stalled band
        api.backtrace_profile_host(aln32, letters, lo + qs, qe - qs + 1, t[ts:te + 1], best + 1)
