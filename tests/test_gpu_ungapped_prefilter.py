"""ungappedprefilter / --prefilter-mode 1 on the GPU: every query's hit list of mk_ungapped_prefilter (mk_ungapped.hip) against the list built from the
literal byte loop of test_ungapped_prefilter_host plus the verdict, sort and cut written out here, at the shapes where the kernel changes path; the
commands against each other."""
import ctypes
import subprocess

import numpy as np
import pytest

from test_ungapped_prefilter_host import reference, saturating_pair

pytestmark = pytest.mark.gpu


def _offsets(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)


@pytest.fixture(scope="module")
def world(gpu_api):
    """(db, batch, queries, targets, keys, {bias on: score of every pair by the byte loop})"""
    api, rs = gpu_api, np.random.RandomState(23)
    C, T, GS, GL = api.UNG_DIAGS, api.UNG_ROW_TILE, api.UNG_GROUP_SHORT * api.UNG_DIAGS, api.UNG_GROUP_LONG * api.UNG_DIAGS
    rnd = lambda n: rs.randint(0, 20, int(n)).astype(np.uint8)
    sat_q, sat_t, _, _ = saturating_pair(rs)
    # every row-block and row-tile edge and a count that is no multiple of the group.  The batch is sorted by length before groups of four form: this one
    # runs as (1, 1, 7, 8), (9, 33, 64, 64), (64, 90, 127, 128), (129, 259); lengths 1 and 64 in ONE group: test_packed_halves_of_lengths_1_and_64
    queries = [rnd(n) for n in (1, C - 1, C, C + 1, T - 1, T, T + 1, 2 * T + 3, 1, 64, 64, 33, 90)] + [sat_q]
    probe = np.concatenate([rnd(9), queries[7][40:200], rnd(13)])                          # the probe pair's target: first and last of the database
    targets = [probe, rnd(0), rnd(1)]
    # L + Lq - 1 = G C - 1, G C, G C + 1 for both lane-group shapes (Lq = C and Lq = two tiles + 3)
    targets += [rnd(GS - C + 1 + d) for d in (-1, 0, 1)] + [rnd(GL - (2 * T + 3) + 1 + d) for d in (-1, 0, 1)]
    targets += [sat_t, queries[12], rnd(10), queries[12]]                                  # a short target between two copies of a query
    for k in range(24):                                                                    # mutated pieces of the queries inside random targets
        q = queries[int(rs.randint(1, len(queries)))]
        piece = np.array(q[:int(rs.randint(1, len(q) + 1))])
        piece[rs.rand(len(piece)) < 0.3] = rs.randint(0, 20)
        targets.append(np.concatenate([rnd(rs.randint(0, 60)), piece, rnd(rs.randint(0, 60))])[:300])
    targets.append(probe)
    t_off = _offsets(targets)
    assert {int(o) % 4 for o in t_off[:-1]} == {0, 1, 2, 3}                                # target starts on all four residues of a dword
    db = api.TargetDB.sequences(np.concatenate(targets), t_off)
    keys = np.arange(len(targets), dtype=np.uint32)[::-1].copy() * 3 + 5                   # descending: index order is not key order
    assert api.lib().mk_targetdb_set_keys(db.h, keys.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(keys))) == 0
    q_off = _offsets(queries)
    q = api.Queries.from_codes(np.concatenate(queries), q_off)
    sb = q.derived()[2]
    scores = {on: [[reference(qq, t, sb[int(q_off[i]):int(q_off[i + 1])] if on else None) for t in targets] for i, qq in enumerate(queries)] for on in (1, 0)}
    assert scores[0][13][9] == 251 and scores[1][12][11] < 60                              # the saturating pair; the short target between the copies
    return db, q, queries, targets, keys, scores


def expected(scores, queries, targets, keys, p):
    """per query: pairs that can be covered, score > threshold, score descending then key ascending, the first max_seqs"""
    c, out = np.float32(p.cov_thr), []
    for qi, q in enumerate(queries):
        hits = []
        for ti, t in enumerate(targets):
            with np.errstate(divide="ignore", invalid="ignore"):
                ql, tl = np.float32(len(q)), np.float32(len(t))
                covered = {0: ql / tl >= c and tl / ql >= c, 2: tl / ql >= c}[p.cov_mode]
            if covered and scores[qi][ti] > p.min_ungapped_score:
                hits.append((-scores[qi][ti], int(keys[ti]), ti))
        out.append([(ti, -s) for s, _, ti in sorted(hits)[:p.max_seqs]])
    return out


# name: (parameters, score budget in bytes or None)
VARIANTS = {"defaults": ({}, None), "no bias": (dict(comp_bias_corr=0), None), "cut": (dict(max_seqs=5, min_ungapped_score=0), None),
            "threshold": (dict(min_ungapped_score=None), None), "filter": (dict(cov_thr=0.8, cov_mode=0), None),
            "chunks": (dict(max_seqs=7), 4 * 16)}


@pytest.mark.parametrize("group", [8, 64])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_hit_lists_equal_the_byte_loop(gpu_api, world, monkeypatch, variant, group):
    api, (db, q, queries, targets, keys, scores) = gpu_api, world
    flags, budget = VARIANTS[variant]
    p = api.default_params()
    for k, v in flags.items():
        setattr(p, k, v if v is not None else sorted(s for row in scores[1] for s in row if s > 15)[40])    # an occurring score: strictness
    monkeypatch.setenv("MK_UNGAPPED_GROUP", str(group))
    if budget:
        monkeypatch.setenv("MK_UNGAPPED_SCORE_BUDGET", str(budget))                         # 16 targets x 4 queries: several chunks both ways
    hits, off = api.ungapped_prefilter(db, q, p)
    want = expected(scores[1 if p.comp_bias_corr else 0], queries, targets, keys, p)
    got = [[(int(h["seq_id"]), int(h["pref_score"])) for h in hits[int(off[i]):int(off[i + 1])]] for i in range(len(queries))]
    bad = [(i, got[i][:4], want[i][:4]) for i in range(len(queries)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:3])
    assert all(int(h["diagonal"]) == 0 for h in hits) and sum(len(w) for w in want) > (20 if variant != "filter" else 3)
    assert api.kernel_stats(reset=True)["ungapped_prefilter"]["cells"] > 10000


@pytest.mark.parametrize("group", [8, 64])
@pytest.mark.parametrize("lengths", [(64, 1), (1, 64, 64, 1)])
def test_packed_halves_of_lengths_1_and_64(gpu_api, world, monkeypatch, lengths, group):
    """a batch that is ONE group of packed halves after the sort by length, (1, 64) or (1, 1, 64, 64): 63 rows behind the short queries' end add 0"""
    api, (db, _, _, targets, keys, _) = gpu_api, world
    queries = [np.array(targets[9][37:37 + n]) if n > 1 else np.array([18], dtype=np.uint8) for n in lengths]      # (W alone; the 64s saturate on target 9)
    q_off = _offsets(queries)
    batch = api.Queries.from_codes(np.concatenate(queries), q_off)
    sb = batch.derived()[2]
    scores = [[reference(qq, t, sb[int(q_off[i]):int(q_off[i + 1])]) for t in targets] for i, qq in enumerate(queries)]
    p = api.default_params()
    p.min_ungapped_score = 3                                                               # the 1-residue queries keep their identities
    monkeypatch.setenv("MK_UNGAPPED_GROUP", str(group))
    hits, off = api.ungapped_prefilter(db, batch, p)
    want = expected(scores, queries, targets, keys, p)
    assert [[(int(h["seq_id"]), int(h["pref_score"])) for h in hits[int(off[i]):int(off[i + 1])]] for i in range(len(queries))] == want
    k = lengths.index(64)                                                                  # its cap: 255 - |matrix minimum| - |bias minimum|
    assert all(len(w) > 3 for w in want) and want[k][0][1] == 251 + min(0, int(sb[int(q_off[k]):int(q_off[k + 1])].min()))


def test_cut_keeps_the_smallest_keys_of_a_tie(gpu_api):
    """max_seqs 5 against 40 targets of which 12 tie at the cut score, DB keys descending"""
    api, rs = gpu_api, np.random.RandomState(4)
    q = rs.randint(0, 20, 40).astype(np.uint8)
    tie = np.concatenate([rs.randint(0, 20, 20), q[5:19], rs.randint(0, 20, 9)]).astype(np.uint8)
    targets = [np.concatenate([rs.randint(0, 20, 7), q[:n]]).astype(np.uint8) for n in (40, 34, 28)] + [tie] * 12 + [rs.randint(0, 20, 60).astype(np.uint8) for _ in range(25)]
    order = rs.permutation(40)
    targets = [targets[k] for k in order]
    keys = (np.arange(40, dtype=np.uint32)[::-1] + 100).copy()
    db = api.TargetDB.sequences(np.concatenate(targets), _offsets(targets))
    assert api.lib().mk_targetdb_set_keys(db.h, keys.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(40)) == 0
    batch = api.Queries.from_codes(q, _offsets([q]))
    p = api.default_params()
    p.max_seqs = 5
    sb = batch.derived()[2]
    scores = [[reference(q, t, sb) for t in targets]]
    want = expected(scores, [q], targets, keys, p)[0]
    assert scores[0].count(want[-1][1]) == 12 and want[2][1] > want[3][1] == want[4][1]      # three above the tie, two of the twelve stay
    hits, off = api.ungapped_prefilter(db, batch, p)
    assert [(int(h["seq_id"]), int(h["pref_score"])) for h in hits] == want


def test_refusals_by_name(gpu_api, world):
    from test_gpu_profile import _golden_inputs
    api, db = gpu_api, world[0]
    with pytest.raises(api.MkError, match="error -3.*profile"):
        api.ungapped_prefilter(db, api.Profiles(_golden_inputs()[1][:1]))


def test_search_prefilter_mode_1_is_the_two_commands(gpu_api, tmp_path):
    """`search --prefilter-mode 1` writes the alignment DB of `ungappedprefilter` followed by `align`; the refused corners name their flag"""
    from metaeuk_amd import build
    from test_backtrace_host import _lines
    from test_gpu_backtrace import _write_seq_db
    t = str(tmp_path) + "/"
    frags = [l.rsplit("\t", 1)[1] for l in _lines("e2e_process_orfs.txt.gz")][:400]
    _write_seq_db(t + "targets", _lines("e2e_targets.txt.gz")); _write_seq_db(t + "aa_6f", frags)
    run = lambda *argv: subprocess.run([build.BIN] + list(argv), stderr=subprocess.PIPE, timeout=120)
    common = ["--max-seqs", "20", "-e", "100", "--alignment-mode", "2", "--threads", "4"]
    assert run("search", t + "aa_6f", t + "targets", t + "srch", t + "tmp", "--prefilter-mode", "1", *common).returncode == 0
    assert run("ungappedprefilter", t + "aa_6f", t + "targets", t + "pref", "--max-seqs", "20", "--threads", "4").returncode == 0
    assert run("align", t + "aa_6f", t + "targets", t + "pref", t + "aln", *common[2:]).returncode == 0
    assert open(t + "srch", "rb").read() == open(t + "aln", "rb").read() and len(open(t + "aln", "rb").read()) > 2000
    assert open(t + "pref.dbtype", "rb").read() == (7).to_bytes(4, "little")
    for bad in (["search", t + "aa_6f", t + "targets", t + "bad", t + "tmp", "--alignment-mode", "2", "--prefilter-mode", "3"],
                ["search", t + "aa_6f", t + "targets", t + "bad", t + "tmp", "--alignment-mode", "2", "--prefilter-mode", "1", "--split", "2"],
                ["predictexons", t + "aa_6f", t + "targets", t + "bad", t + "tmp", "--prefilter-mode", "1"],
                ["ungappedprefilter", t + "aa_6f", t + "targets", t + "bad", "--taxon-list", "9606"]):
        r = run(*bad)
        assert r.returncode != 0 and bad[-2].encode() in r.stderr, (bad, r.stderr[-300:])
