"""--alt-ali without a GPU: mk_alt_alignments_host (csrc/mk_altali.hpp, scalar Gotoh on the masked target) against the plain C oracle run on the
target STRING with the chain's mask written as X, round by round, and the chain's stop against the criteria restated in numpy float32."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle

AA = "ACDEFGHIKLMNPQRSTVWY"
F = np.float32
FLAGS = {"e001": dict(evalue_thr=0.001, min_aln_len=5), "open": dict(evalue_thr=1e9, min_aln_len=0),
         "c05 id03": dict(evalue_thr=0.001, min_aln_len=5, cov_thr=0.5, cov_mode=2, seq_id_thr=0.3)}


def params_of(api, flags):
    p = api.default_params()
    for k, v in FLAGS[flags].items():
        setattr(p, k, v)
    return p


@functools.lru_cache(None)
def workload():
    """(queries, targets, per query the targets of its list).  Copies of a query keep their first and last five residues, so an alignment spans
    the copy exactly and the mask edges sit where the spacers put them."""
    rs = np.random.RandomState(7)
    rnd = lambda n: "".join(AA[i] for i in rs.randint(0, 20, n))

    def mut(s, rate):
        return s[:5] + "".join(c if rs.rand() > rate else AA[rs.randint(20)] for c in s[5:-5]) + s[-5:] if len(s) > 12 else s
    queries, targets, lists = [], [], []

    def add(q, ts):
        queries.append(q); lists.append(list(range(len(targets), len(targets) + len(ts)))); targets.extend(ts)
    q0 = rnd(40)
    # a three-copy repeat, differently mutated copies; two origins on one target (the list names it twice)
    add(q0, [rnd(7) + mut(q0, 0.1) + rnd(25) + mut(q0, 0.2) + rnd(30) + mut(q0, 0.3) + rnd(9)])
    lists[-1] = lists[-1] * 2
    # mask edges at target positions 0, 1, 2, 3 (every offset mod 4), around the 32-column fetch block, and an end at tLen - 1
    q1 = rnd(40)
    add(q1, [rnd(p) + mut(q1, 0.1) + rnd(11 + p % 3) + mut(q1, 0.15) for p in (0, 1, 2, 3, 30, 31, 32, 33)])
    # the unmasked last residue is used again: two copies that overlap in one residue
    q2 = rnd(39); q2 = q2 + q2[0]
    add(q2, [rnd(6) + q2 + mut(q2, 0.1)[1:] + rnd(6)])
    # rows: 1 (a one-column origin: the empty mask), 15, 64, 65, 300 (the 256-column block of the wide shape), 1 100 (row tiles)
    add("W", [rnd(20).replace("W", "A") + "W" + rnd(9).replace("W", "A")])
    for n, pre in ((15, 3), (64, 5), (65, 2), (300, 255), (300, 257), (1100, 9)):
        q = rnd(n)
        second = mut(q, 0.2) if n > 15 else q[:7] + AA[(AA.index(q[7]) + 1) % 20] + q[8:]       # (15 rows: one planted substitution, never a tie)
        add(q, [rnd(pre) + mut(q, 0.1 if n > 15 else 0.0) + rnd(13) + second + rnd(4)])
    add(rnd(40), [])                                         # a query with no alignments
    return queries, targets, lists


def criteria(api, p, ev, score, qs, qe, ts, te, q_len, t_len):
    """Alignment::checkCriteria on the record of Matcher::getSWResult, in numpy float32 / double"""
    cov = lambda s, e, n: F(min(n, max(s, e)) - min(s, e) + 1) / F(n)
    a = api.Alignment()
    a.qcov, a.dbcov = cov(qs, qe, q_len), cov(ts, te, t_len)
    a.seq_id = max(F(0), min(F(1), F(float(F(score) / F(max(qe - qs, te - ts, 1))) * 0.1656 + 0.1141)))
    aln_len = max(qe - qs, te - ts) + 1
    return oracle.lib().mko_evalue(C.byref(ev), C.c_double(score), C.c_double(q_len)) <= p.evalue_thr and aln_len >= p.min_aln_len and api.result_filter(p, q_len, t_len, a)


def oracle_chain(api, p, ev, q, t, n):
    """the origin and the chain's alternatives as the oracle finds them: [(score, q_start, q_end, db_start, db_end)], origin first; None = no origin"""
    out, tm = [], t
    for _ in range(n + 1):
        s, qe, te, qs, ts, mismatch = oracle.sw(q, tm)
        assert not mismatch
        if s <= 0 or not criteria(api, p, ev, s, qs, qe, ts, te, len(q), len(t)):
            break
        out.append((s, qs, qe, ts, te))
        tm = tm[:ts] + "X" * (te - ts) + tm[te:]             # [db_start, db_end): the last aligned residue stays
    return out or None


@pytest.mark.parametrize("flags,n", [("e001", 1), ("e001", 2), ("e001", 5), ("open", 3), ("c05 id03", 2)])
def test_twin_equals_the_oracle_on_the_masked_string(flags, n):
    from metaeuk_amd import api
    queries, targets, lists = workload()
    p, ev = params_of(api, flags), (C.c_double * 32)()
    oracle.lib().mko_evalue.restype = C.c_double
    db_res = sum(len(t) for t in targets)
    oracle.lib().mko_evaluer_init(C.byref(ev), C.c_uint64(db_res))
    t_codes = api.encode(targets)
    chains = 0
    for qi, q in enumerate(queries):
        kept = []
        for ti in sorted(set(lists[qi])):
            want = oracle_chain(api, p, ev, q, targets[ti], n)
            if want is None:
                continue
            origin = api.Alignment()
            origin.db_key, origin.db_start, origin.db_end = ti, want[0][3], want[0][4]
            got = api.alt_alignments_host(api.encode([q])[0][:len(q)], oracle.query_bias8(q), t_codes[0][int(t_codes[1][ti]):int(t_codes[1][ti + 1])], origin, db_res, p, n)
            assert [(a.raw_score, a.q_start, a.q_end, a.db_start, a.db_end) for a in got] == want[1:], (qi, ti)
            assert all(a.db_key == ti and a.q_len == len(q) and a.db_len == len(targets[ti]) for a in got)
            kept += [(a.evalue, a.raw_score, a.db_len, a.db_key) for a in got] + [(None,) + want[0][:1] + (len(targets[ti]), ti)]
            chains += len(want) > 1
            if flags == "open" and q == "W":
                assert want[1:] == [want[0]] * n             # the empty mask: the same record again, N times
            if q[0] == q[-1] and len(q) == 40 and flags != "c05 id03":
                assert want[1][3] == want[0][4]              # the second alignment starts on the unmasked last residue of the first
        # ("open" repeats a record by design; elsewhere the kept records of a query never tie on score, db_len and key, so the order is the reference's)
        if flags != "open":
            assert len({k[1:] for k in kept}) == len(kept), qi
    assert chains >= 10
    if flags == "e001" and n == 5:                           # the three-copy repeat: two alternatives, then a rejection ends the chain before 5
        assert len(oracle_chain(api, p, ev, queries[0], targets[0], 5)) == 3
