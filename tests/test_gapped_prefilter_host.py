"""The exhaustive gapped prefilter on the host: mk_gapped_prefilter_host (the Gotoh cell step of mk_gapped.hpp as a plain row loop) against a row loop in
Python integers and against oracle.sw, on small pairs and the named corners; and the world the GPU file scores, with its sanity assertions."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import oracle

AA = "ACDEFGHIKLMNPQRSTVWY"


def gotoh(q, t, bias8):
    """H = max(0, H(i-1, j-1) + s, E, F); E(i, j+1) = max(E - 1, H - 11); F(i+1, j) = max(F - 1, H - 11); additions capped at 32767"""
    m = oracle.aln_matrix().astype(int)
    H, F, best = [0] * (len(t) + 1), [-10 ** 9] * (len(t) + 1), 0
    for i in range(len(q)):
        diag, E = 0, -10 ** 9
        for j in range(1, len(t) + 1):
            h = max(0, min(diag + int(m[t[j - 1], q[i]]) + int(bias8[i]), 32767), E, F[j])
            diag, H[j], best = H[j], h, max(best, h)
            E, F[j] = max(E - 1, h - 11), max(F[j] - 1, h - 11)
    return best


def rnd(rs, n):
    return "".join(AA[k] for k in rs.randint(0, 20, int(n)))


def golden_saturating_pair():
    """the 6500-residue identical pair of the sw2_* golden: the reference's word pass saturates"""
    rd = lambda f: gzip.open(os.path.join(os.path.dirname(__file__), "golden", f), "rt").read().split("\n")
    return rd("sw2_queries.txt.gz")[10], rd("sw2_targets.txt.gz")[10]


def gap_pairs(rs):
    """pairs whose optimum needs a gap of 2 .. 4 residues, in the query (a horizontal gap) and in the target (a vertical one)"""
    out = []
    for d in (2, 3, 4):
        q = rnd(rs, 40)
        out += [(q, rnd(rs, 5) + q[:20] + rnd(rs, d) + q[20:] + rnd(rs, 3)), (q, rnd(rs, 4) + q[:18] + q[18 + d:])]
    return out


@pytest.mark.parametrize("scale", [1.0, 0.0])
def test_twin_equals_the_row_loop_and_the_oracle(scale):
    from metaeuk_amd import api
    rs = np.random.RandomState(11)
    pairs = [(rnd(rs, rs.randint(1, 50)), rnd(rs, rs.randint(0, 70))) for _ in range(24)] + gap_pairs(rs)
    pairs += [(rnd(rs, 30), ""), ("W", rnd(rs, 20) + "W"), (pairs[0][0], pairs[0][0])]        # an empty target, a 1-residue query, identity
    for k, (q, t) in enumerate(pairs):
        qc, tc, cb = api.encode([q])[0][:len(q)], api.encode([t])[0][:len(t)], oracle.query_bias8(q, scale)
        got = api.gapped_prefilter_host(qc, tc, cb if scale else None)
        assert got == gotoh(qc, tc, cb) == oracle.sw(q, t, bias_scale=scale, with_start=False)[0], (k, q, t)
        if 24 <= k < 30:                                                                   # the gap is needed: the gapless sibling scores less
            assert got > api.ungapped_prefilter_host(qc, tc, cb if scale else None), (k, q, t)


def test_saturating_pair_scores_the_cap():
    from metaeuk_amd import api
    q, t = golden_saturating_pair()
    assert api.gapped_prefilter_host(api.encode([q])[0], api.encode([t])[0], oracle.query_bias8(q)) == 32767 == oracle.sw(q, t, with_start=False)[0]


def evaluer(targets):
    """e-value of (score, query length) against these targets: the gapped parameter set, the database's residues"""
    ev = (C.c_double * 32)()
    oracle.lib().mko_evalue.restype = C.c_double
    oracle.lib().mko_evaluer_init(C.byref(ev), C.c_uint64(sum(len(t) for t in targets)))
    return lambda s, ql: oracle.lib().mko_evalue(C.byref(ev), C.c_double(s), C.c_double(ql))


def build_world():
    """queries, targets (strings), DB keys, {bias on: oracle.sw score of every pair}, e-value of (score, query length), at the kernel's edges"""
    from metaeuk_amd import api
    rs = np.random.RandomState(29)
    G, rows = api.GAP_GROUP, [api.GAP_ROWS_0, api.GAP_ROWS_1, api.GAP_ROWS_2]
    big = G * rows[-1]
    lens = [1, rows[0] - 1, rows[0], rows[0] + 1] + [G * r + d for r in rows for d in (-1, 0, 1)] + [2 * big + 3, 90]
    assert len(lens) % 2 == 1 and big + 1 in lens                                          # a lone half; the first length that needs row tiles
    queries = [rnd(rs, n) for n in lens]
    targets = [rnd(rs, n) for n in (0, 1, G - 1, G, G + 1)]                                # shorter than the ramp
    for q, r in [(queries[lens.index(G * r)], r) for r in rows] + [(queries[-2], rows[-1])]:
        # a deletion across a lane's row boundary (a vertical gap), an insertion (a horizontal one), 2 .. 5 residues; for the long query the deletion
        # crosses the row-tile boundary as well
        cut, d = (big if len(q) > big else 3 * r) - 1, int(rs.randint(2, 6))
        targets += [rnd(rs, rs.randint(0, 9)) + q[:cut] + q[cut + d:] + rnd(rs, 5), rnd(rs, 6) + q[:cut + 1] + rnd(rs, d) + q[cut + 1:]]
    q64 = queries[lens.index(64)]
    targets += [q64 + rnd(rs, 10) + q64]                                                   # a short stretch between two copies of a query
    targets += [rnd(rs, 7) + q64[10:40] + rnd(rs, 11)] * 4                                 # a tie of four at the cut of max_seqs 5
    targets += [rnd(rs, rs.randint(20, 300)) for _ in range(30)]
    starts = np.cumsum([0] + [len(t) for t in targets])[:-1]
    assert {int(o) % 4 for o in starts} == {0, 1, 2, 3}                                    # target starts on all four bytes of a dword
    keys = (np.arange(len(targets), dtype=np.uint32)[::-1] * 3 + 5).copy()                 # descending: index order is not key order
    scores = {on: [[oracle.sw(q, t, bias_scale=float(on), with_start=False)[0] for t in targets] for q in queries] for on in (1, 0)}
    return queries, targets, keys, scores, evaluer(targets)


def expected(world, p, bias_on=1):
    """per query: pairs that can be covered, score > threshold, e-value <= threshold, score descending then key ascending, the first max_seqs"""
    queries, targets, keys, scores, evalue = world
    c, out = np.float32(p.cov_thr), []
    for qi, q in enumerate(queries):
        hits = []
        for ti, t in enumerate(targets):
            with np.errstate(divide="ignore", invalid="ignore"):
                ql, tl = np.float32(len(q)), np.float32(len(t))
                covered = {0: ql / tl >= c and tl / ql >= c, 2: tl / ql >= c}[p.cov_mode]
            s = scores[bias_on][qi][ti]
            if covered and s > p.min_ungapped_score and (p.evalue_thr >= 1.7e308 or evalue(s, len(q)) <= p.evalue_thr):
                hits.append((-s, int(keys[ti]), ti))
        out.append([(ti, -s) for s, _, ti in sorted(hits)[:p.max_seqs]])
    return out


def test_world_is_sharp():
    """what the GPU file relies on, from the reference scores alone: gaps are needed, a tie at the cut, pairs that fail one verdict only"""
    from metaeuk_amd import api
    world = queries, targets, keys, scores, evalue = build_world()
    codes = lambda s: api.encode([s])[0][:len(s)]
    for ti in range(5, 13):                                                                # the indel copies: the gapless score is smaller
        qi = max(range(len(queries)), key=lambda k: scores[0][k][ti])
        assert scores[0][qi][ti] > api.ungapped_prefilter_host(codes(queries[qi]), codes(targets[ti])) and len(queries[qi]) >= 32, ti
    p = api.default_params()
    p.max_seqs, p.min_ungapped_score = 5, 0
    full = [sorted((-s for s in row if s > 0)) for row in scores[1]]
    assert any(len(f) > 5 and f[4] == f[5] for f in full) and all(len(w) <= 5 for w in expected(world, p))
    flat = [(s, evalue(s, len(q))) for q, row in zip(queries, scores[1]) for s in row if s > 0]
    assert any(s > 15 and 0.001 < e <= 100 for s, e in flat)                               # fails only the e-value at 0.001
    assert any(s <= 15 and e <= 100 for s, e in flat)                                      # fails only the threshold at -e 100
