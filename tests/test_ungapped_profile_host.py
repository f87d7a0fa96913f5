"""The gapless prefilter of profile queries on the host: mk_ungapped_prefilter_profile_host (the literal byte steps over the int8 alignment profile)
against the byte loop restated here in int64, on golden profiles and the named corners."""
import numpy as np
import pytest


def reference(aln32, t):
    """(score, 255 - bias): S(i, j) = max(0, min(255, S(i-1, j-1) + P[i][t[j]] + bias) - bias) target position by target position, X scoring 0
    in every column, bias from the 20 amino-acid scores of all columns; the maximum over all cells"""
    P = np.array(np.asarray(aln32).reshape(-1, 32)[:, :21], dtype=np.int64)
    P[:, 20] = 0
    bias = abs(min(0, int(P[:, :20].min())))
    prev, best = np.zeros(len(P) + 1, dtype=np.int64), 0             # prev[i + 1] = S(i, j - 1); prev[0] = the column in front of the profile
    for a in np.asarray(t, dtype=np.int64):
        cur = np.zeros(len(P) + 1, dtype=np.int64)
        cur[1:] = np.maximum(0, np.minimum(255, prev[:-1] + P[:, min(int(a), 20)] + bias) - bias)
        best, prev = max(best, int(cur.max())), cur
    return best, 255 - bias


def _cases():
    """name -> (aln32 with one favoured residue per column, target); golden profiles against golden fragments"""
    import oracle
    from metaeuk_amd import api
    from test_gpu_profile import _golden_inputs
    rs, out = np.random.RandomState(11), {}
    rnd = lambda n: rs.randint(0, 20, n).astype(np.uint8)
    for n in (1, 7, 8, 9, 64):
        aln = np.zeros((n, 32), dtype=np.int8)
        aln[:, :20] = rs.randint(-6, 2, (n, 20))
        fav = rnd(n)
        aln[np.arange(n), fav] = rs.randint(3, 10, n)
        out["%d columns" % n] = (aln, np.concatenate([rnd(37), fav, rnd(50)]))             # (64 columns: the pair saturates)
    out["empty target"] = (aln, rnd(0))
    t = np.array(fav)
    t[::3], t[1::9] = 20, 23                                                               # X, and a code above 20 that is read as X
    out["X in the target"] = (aln, t)
    _, entries, frags, _, _ = _golden_inputs()
    res, off = api.encode(frags[:40])
    for k, e in enumerate(entries[:4]):
        a = np.zeros(((len(e) - 1) // 25, 32), dtype=np.int8)
        a[:, :21] = oracle.profile_arrays(e, len(a))[2]
        for f in range(40):
            out["golden %d x %d" % (k, f)] = (a, res[int(off[f]):int(off[f + 1])])
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_equals_the_byte_loop(name):
    from metaeuk_amd import api
    aln, t = CASES[name]
    want, cap = reference(aln, t)
    assert api.ungapped_prefilter_profile_host(aln, t) == want
    assert want == {"64 columns": cap, "empty target": 0}.get(name, want) and (name == "empty target" or want > 0)
