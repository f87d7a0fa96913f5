"""The prefilter on the hand-made cases of tests/pf_cases.py, query by query against the oracle, under every front end: the double-diagonal rule
as stream_kernel (pass 2), wide_kernel and double_hit_count_kernel / double_hit_emit_kernel each restate it, the dword scorer of
diag_score_kernel at every (alignment, tail) shape, and the per-query tiers with a query at maxpos and at maxpos + 1 k-mer starts.
tests/test_pf_cases_host.py holds the conditions under which this cannot pass by accident."""
import tempfile

import pytest

import oracle
import pf_cases as pc

pytestmark = pytest.mark.gpu
FRONTS = ["fused", "fused-tiny", "wide", "wide-tiny", "global"]


@pytest.fixture(params=FRONTS)
def front(request, monkeypatch):
    """front end of the prefilter (as pf_path of tests/test_gpu_parity.py); the library reads the variables on every call"""
    return _set_front(monkeypatch, request.param)


def _set_front(monkeypatch, name):
    monkeypatch.setenv("MK_PREFILTER_PATH", name.split("-")[0])
    monkeypatch.setenv("MK_PREFILTER_TIERS", "tiny" if name.endswith("-tiny") else "default")
    return name


_ORACLE = {}


def _oracle_blocks(api, name):
    """the oracle's prefilter and alignment blocks of a group, computed once per session"""
    if name not in _ORACLE:
        cs = pc.group(name)
        with tempfile.TemporaryDirectory() as tmp:
            _ORACLE[name] = oracle.run_pipeline(cs.targets, cs.queries, tmp, extra=["--l2", str(api.default_params().host_l2_bytes)])
    return _ORACLE[name]


def _check(cs, got, want, form):
    """got / want: the formatted hit list of every query.  A difference names the case, its designed hits and both lines"""
    bad = []
    for q, (g, w) in enumerate(zip(got, want)):
        if g == w:
            continue
        gl, wl = ({int(l.split("\t")[0]): l for l in b.splitlines()} for b in (g, w))
        diff = [t for t in sorted(set(gl) | set(wl)) if gl.get(t) != wl.get(t)]
        for t in diff:
            bad.append("%s [%s]: stage %r, oracle %r (target, pref_score, diagonal)" % (cs.describe(q, t), form, gl.get(t), wl.get(t)))
        if not diff:
            bad.append("%s query %d [%s]: the same lines in another order:\nstage\n%soracle\n%s" % (cs.name, q, form, g, w))
    assert not bad, "%d pairs differ from the oracle:\n%s" % (len(bad), "\n".join(bad[:8]))
    assert len(got) == len(want) == len(cs.queries)


def _prefilter(api, cs):
    params = api.default_params()
    db = api.TargetDB(cs.targets, params)
    q = api.Queries(cs.queries, params)
    try:
        hits, hoff = api.prefilter(db, q)
        return [api.format_hits(hits, int(hoff[i]), int(hoff[i + 1])) for i in range(len(cs.queries))], q.off.copy(), db.off.copy()
    finally:
        q.close()
        db.close()


@pytest.mark.parametrize("name", ["R12", "R3", "S"])
def test_cases_under_every_front_end(gpu_api, front, name):
    """(A front end hands a query it cannot hold to the global path: under wide-tiny, 64 k-mer starts at the most, only the chains of 2 and 5
    segments of R12 stay in wide_kernel; R3, S and the longer chains are the global path's there.)"""
    cs = pc.group(name)
    got, _, _ = _prefilter(gpu_api, cs)
    _check(cs, got, _oracle_blocks(gpu_api, name)[0], front)
    present = sum(1 for c in cs.cases if c.expect != "absent")
    assert sum(len(b.splitlines()) for b in got) >= present > 0


def test_scorer_shapes_from_the_device_offsets(gpu_api):
    """the (query alignment, target alignment, tail) coverage of the S group once more, from the offsets the library was given for the device's
    residue arrays (Queries.off, TargetDB.off: V.q_off / V.t_off of diag_score_kernel; the arrays themselves start on allocation boundaries)"""
    api = gpu_api
    cs = pc.group("S")
    params = api.default_params()
    db = api.TargetDB(cs.targets, params)
    q = api.Queries(cs.queries, params)
    try:
        assert len(q.off) == len(cs.queries) + 1 and len(db.off) == len(cs.targets) + 1
        pos, neg = pc.scorer_coverage(cs, q.off, db.off)
    finally:
        q.close()
        db.close()
    assert pos == {(a, b, c) for a in range(4) for b in range(4) for c in range(4)}
    assert {(a, b) for a, b, _ in neg} == {(a, b) for a in range(4) for b in range(4)}


def test_scorer_cases_through_search(gpu_api, front):
    """the S group through mk_search: the back end beside the alignment stage"""
    api = gpu_api
    cs = pc.group("S")
    params = api.default_params()
    db = api.TargetDB(cs.targets, params)
    q = api.Queries(cs.queries, params)
    try:
        (hits, hoff), (alns, aoff) = api.search(db, q)
        got = [api.format_hits(hits, int(hoff[i]), int(hoff[i + 1])) for i in range(len(cs.queries))]
        galn = [api.format_alignments(alns, int(aoff[i]), int(aoff[i + 1])) for i in range(len(cs.queries))]
    finally:
        q.close()
        db.close()
    opref, oaln = _oracle_blocks(api, "S")
    _check(cs, got, opref, front + ", search")
    assert galn == oaln


@pytest.mark.parametrize("form", ["fused", "fused-tiny"])
def test_tier_edges(gpu_api, monkeypatch, form):
    """plain random queries of maxpos and maxpos + 1 k-mer starts for every limit of both tier sets: the oracle's hit lists, and the launches a
    query at either side of every limit of this set needs -- each tier's own and, behind the last limit, the global path -- are booked.  A
    tier is also left for the number of similar k-mers, and at the miniature shapes that decides for plain random residues: which tier RAN
    which query is asserted on the queries of test_the_limit_decides_the_tier."""
    api = gpu_api
    _set_front(monkeypatch, form)
    cs = pc.group("T")
    api.kernel_stats(reset=True)
    got, _, _ = _prefilter(api, cs)
    stats = api.kernel_stats()
    _check(cs, got, _oracle_blocks(api, "T")[0], form)
    prod, mini = pc.tiers()
    tiers = mini if form.endswith("-tiny") else prod
    lengths = {len(s) for s in cs.queries}
    for cap, _, maxpos, _ in tiers:
        assert maxpos + 9 in lengths and maxpos + 10 in lengths
    names = [pc.tier_kernel_name(cap) for cap, _, _, _ in tiers] + [pc.global_kernel_name()]
    print("T [%s]: %s" % (form, {n: stats.get(n) for n in names}))
    for n in names:
        assert n in stats and stats[n]["launches"] >= 1, (n, sorted(stats))


def _alone(api, db, seq, tier_set):
    """one query in a prefilter call of its own -> its formatted hit list, the similar k-mers every tier's launch booked as its work (the total
    of the queries it ran, mk_prefilter.hip:825 and :2894), the launches of the global path's rule"""
    q = api.Queries([seq], api.default_params())
    try:
        api.kernel_stats(reset=True)
        hits, hoff = api.prefilter(db, q)
        stats = api.kernel_stats()
        block = api.format_hits(hits, int(hoff[0]), int(hoff[1]))
    finally:
        q.close()
    work = [stats.get(pc.tier_kernel_name(cap), {}).get("cells", 0.0) for cap, _, _, _ in tier_set]
    return block, work, stats.get(pc.global_kernel_name(), {}).get("launches", 0)


def _check_alone(api, cs, q, db, tier_set, tier, form):
    block, work, glob = _alone(api, db, cs.queries[q], tier_set)
    print("%s query %d (%d residues) [%s]: similar k-mers run per tier %s, global launches %d" % (cs.name, q, len(cs.queries[q]), form, work, glob))
    assert block == _oracle_blocks(api, cs.name)[0][q], "%s query %d [%s]:\nstage\n%soracle\n%s" % (cs.name, q, form, block, _oracle_blocks(api, cs.name)[0][q])
    assert [w > 0 for w in work] == [t == tier for t in range(len(tier_set))] and (glob >= 1) == (tier is None), \
        "%s query %d (%d residues) [%s] belongs to %s: similar k-mers run per tier %s, global launches %d" % (
            cs.name, q, len(cs.queries[q]), form, "the global path" if tier is None else "tier %d" % tier, work, glob)


@pytest.mark.parametrize("form", ["fused", "fused-tiny"])
def test_the_limit_decides_the_tier(gpu_api, monkeypatch, form):
    """which tier RAN a query of maxpos and of maxpos + 1 k-mer starts, for every limit of both tier sets.  The queries of TL have one k-mer and
    too few similar k-mers for any limit[t] (tests/test_pf_cases_host.py), so the comparison with maxpos[t] in tier_classify_kernel decides:
    each runs alone, and the tier whose launch booked its similar k-mers as work must be the first with maxpos >= its k-mer starts and no
    other -- the global path's rule behind the last.  The third miniature tier has the maxpos of the second: the queries of TK reach its
    edge by their similar k-mers, on a database the tiers have not sized yet"""
    api = gpu_api
    _set_front(monkeypatch, form)
    prod, mini = pc.tiers()
    tier_set = mini if form.endswith("-tiny") else prod
    cs = pc.group("TL")
    db = api.TargetDB(cs.targets, api.default_params())
    reached = set()
    try:
        for c in cs.cases:
            tier = pc.tier_by_length(tier_set, len(cs.queries[c.q]) - 9)
            _check_alone(api, cs, c.q, db, tier_set, tier, form)
            reached.add(tier)
    finally:
        db.close()
    assert reached == ({0, 1, 3, None} if tier_set is mini else {0, 1, 2, 3, None})
    if tier_set is mini:
        tk = pc.group("TK")
        assert len(tk.targets) != len(cs.targets)                        # another database: the sizing learned on TL is dropped (mk_prefilter.hip:2715)
        db = api.TargetDB(tk.targets, api.default_params())
        try:
            _check_alone(api, tk, 0, db, tier_set, 2, form)                # 64 k-mer starts, similar k-mers between limit[1] and limit[2]
            _check_alone(api, tk, 1, db, tier_set, 3, form)                # 65
        finally:
            db.close()
