"""The gapped prefilter of profile queries on the host: mk_gapped_prefilter_profile_host (the Gotoh cell step of mk_gapped.hpp over the int8 alignment
profile) against the recurrence restated here in int64, on the named corners and on golden profiles, where it also equals the oracle's profile SW."""
import numpy as np
import pytest


def reference(aln32, targets):
    """local Gotoh of one profile against every target, int64: H(i, j) = max(0, min(H(i-1, j-1) + P[i][t[j]], 32767), E, F), E(i, j+1) =
    max(E - 1, H - 11) along the target, F(i+1, j) = max(F - 1, H - 11) along the columns, X and every code above 20 scoring 0; the maximum per pair.
    A column's row is computed for all targets and positions at once: with H' = H without its E term, E(i, j) = max over k < j of
    H'(i, k) - 11 - (j - 1 - k) (a gap opened on a cell that came out of a gap is the longer gap), one running maximum of H'(i, k) + k."""
    P = np.array(np.asarray(aln32).reshape(-1, 32)[:, :21], dtype=np.int64)
    P[:, 20] = 0
    n, L = len(targets), max([len(t) for t in targets] + [1])
    codes = np.full((n, L), 21, dtype=np.int64)
    for k, t in enumerate(targets):
        codes[k, :len(t)] = np.minimum(np.asarray(t, dtype=np.int64), 20)
    real, at, j = codes < 21, np.minimum(codes, 20), np.arange(L, dtype=np.int64)
    H, F, best = np.zeros((n, L + 1), dtype=np.int64), np.full((n, L), -10 ** 9, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for col in P:
        h = np.maximum(np.maximum(0, np.minimum(H[:, :-1] + np.where(real, col[at], -10 ** 9), 32767)), F)
        h[:, 1:] = np.maximum(h[:, 1:], np.maximum.accumulate(h + j, axis=1)[:, :-1] - 10 - j[1:])
        F, H[:, 1:] = np.maximum(F - 1, h - 11), h
        best = np.maximum(best, np.where(real, h, 0).max(axis=1))
    return best


def _cases():
    """name -> (aln32, target, oracle score or None): one favoured residue per column; golden profiles against golden fragments"""
    import oracle
    from metaeuk_amd import api
    from test_gpu_profile import _golden_inputs
    rs, out = np.random.RandomState(13), {}
    rnd = lambda n: rs.randint(0, 20, n).astype(np.uint8)
    for n in (1, 3, 4, 5, 40):
        aln = np.zeros((n, 32), dtype=np.int8)
        aln[:, :20], fav = rs.randint(-6, 2, (n, 20)), rnd(n)
        aln[np.arange(n), fav] = rs.randint(6, 12, n)
        out["%d columns" % n] = (aln, np.concatenate([rnd(17), fav, rnd(9)]), None)
    t = np.array(fav)
    t[::3], t[1::9] = 20, 23                                                               # X, and a code above 20 that is read as X
    out.update({"empty target": (aln, rnd(0), None), "X in the target": (aln, t, None),
                "a gap that pays": (aln, np.concatenate([rnd(5), fav[:20], rnd(3), fav[20:], rnd(4)]), None)})      # the consensus with an insertion
    _, entries, frags, _, _ = _golden_inputs()
    res, off = api.encode(frags[:12])
    for k, e in enumerate(entries[:3]):
        a = np.zeros(((len(e) - 1) // 25, 32), dtype=np.int8)
        a[:, :21] = oracle.profile_arrays(e, len(a))[2]
        for f, sw in enumerate(oracle.sw_profile(e, len(a), frags[:12])):
            out["golden %d x %d" % (k, f)] = (a, res[int(off[f]):int(off[f + 1])], sw[0])
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_twin_equals_the_recurrence(name):
    from metaeuk_amd import api
    aln, t, sw = CASES[name]
    want = int(reference(aln, [t])[0])
    assert api.gapped_prefilter_profile_host(aln, t) == want == (want if sw is None else sw) and (want > 0) == (name != "empty target")
    assert name != "a gap that pays" or want > api.ungapped_prefilter_profile_host(aln, t) + 50
