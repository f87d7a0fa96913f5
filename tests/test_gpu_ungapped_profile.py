"""ungappedprefilter with profile queries on the GPU (ungapped_profile_scores_kernel, mk_ungapped.hip): every profile's hit list of
mk_ungapped_prefilter against the list built from the byte loop of test_ungapped_profile_host plus the verdict, sort and cut of the sequence sibling's
test, at the shapes where the kernel changes path; the golden profiles; the refusals; the commands."""
import ctypes
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from test_gpu_ungapped_prefilter import _offsets, expected
from test_ungapped_profile_host import reference

pytestmark = pytest.mark.gpu


def _params(api, **flags):
    p = api.default_params()
    p.profile_search = 1
    for k, v in flags.items():
        setattr(p, k, v)
    return p


def _lists(hits, off, n):
    return [[(int(h["seq_id"]), int(h["pref_score"])) for h in hits[int(off[i]):int(off[i + 1])]] for i in range(n)]


@pytest.fixture(scope="module")
def world(gpu_api):
    """(db, batch, the profiles' aln32 arrays, targets, keys, the score of every pair by the byte loop)"""
    from test_gpu_profile import AA, _synthetic_profile
    api, rs, rng = gpu_api, np.random.RandomState(31), random.Random(31)
    C, T, B = api.UNG_DIAGS, api.UNG_PROF_TILE, api.UNG_PROF_BAND
    rnd = lambda n: rs.randint(0, 20, int(n)).astype(np.uint8)
    short, tiled = 40, 2 * T + 3
    # Lp + Lt - 1 = a band - 1 / 0 / + 1 for the short and for the row-tiled target; more than two bands; the last one saturates on its consensus
    lengths = [1, C - 1, C, C + 1] + [B - short + 1 + d for d in (-1, 0, 1)] + [3 * B - tiled + 1 + d for d in (-1, 0, 1)] + [2 * B + 37, 64]
    entries, cons = zip(*[_synthetic_profile(rng, n) for n in lengths])
    cons = [np.array([AA.index(c) for c in s], dtype=np.uint8) for s in cons]
    targets = [rnd(n) for n in (0, 1, C - 1, C, C + 1, T - 1, T, T + 1)] + [np.concatenate([rnd(100), cons[7][:60], rnd(tiled - 160)]), rnd(short)]
    targets += [np.concatenate([rnd(6), cons[-1], rnd(6)]), cons[10][:90], rnd(10), cons[10][:90]]       # a short target between two copies
    for k in range(30):                                                                    # mutated pieces of the consensus inside random flanks
        c = cons[int(rs.randint(4, len(cons)))]
        piece = np.array(c[:int(rs.randint(len(c) // 2, len(c) + 1))])
        piece[rs.rand(len(piece)) < 0.3] = rs.randint(0, 20)
        targets.append(np.concatenate([rnd(rs.randint(0, 25)), piece, rnd(rs.randint(0, 25))])[:300])
    t_off = _offsets(targets)
    assert {int(o) % 4 for o in t_off[:-1]} == {0, 1, 2, 3}                                # target starts on all four residues of a dword
    db = api.TargetDB.sequences(np.concatenate(targets), t_off, _params(api))
    keys = np.arange(len(targets), dtype=np.uint32)[::-1].copy() * 3 + 5                   # descending: index order is not key order
    assert api.lib().mk_targetdb_set_keys(db.h, keys.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(keys))) == 0
    q = api.Profiles(list(entries), _params(api))
    aln = q.derived()[2]
    profs = [aln[int(q.off[i]):int(q.off[i + 1])] for i in range(q.n)]
    scores = [[reference(a, t)[0] for t in targets] for a in profs]
    assert scores[-1][10] == reference(profs[-1], targets[10])[1] and [len(a) for a in profs] == lengths      # the saturating pair reaches its cap
    return db, q, profs, targets, keys, scores


# name: (parameters, score budget in bytes or None)
VARIANTS = {"defaults": ({}, None), "cut": (dict(max_seqs=5, min_ungapped_score=0), None), "threshold": (dict(min_ungapped_score=None), None),
            "filter": (dict(cov_thr=0.8, cov_mode=0), None), "chunks": (dict(max_seqs=7), 4 * 16)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_hit_lists_equal_the_byte_loop(gpu_api, world, monkeypatch, variant):
    api, (db, q, profs, targets, keys, scores) = gpu_api, world
    flags, budget = VARIANTS[variant]
    p = _params(api)
    for k, v in flags.items():
        setattr(p, k, v if v is not None else sorted(s for row in scores for s in row if s > 15)[40])      # an occurring score: strictness
    if budget:
        monkeypatch.setenv("MK_UNGAPPED_SCORE_BUDGET", str(budget))                         # 16 targets x 4 profiles: several chunks both ways
    api.kernel_stats(reset=True)
    hits, off = api.ungapped_prefilter(db, q, p)
    want, got = expected(scores, profs, targets, keys, p), _lists(hits, off, q.n)
    assert sum(len(w) for w in want) > (20 if variant != "filter" else 3)
    assert got == want, [(i, got[i][:4], want[i][:4]) for i in range(q.n) if got[i] != want[i]][:3]
    assert all(int(h["diagonal"]) == 0 for h in hits) and api.kernel_stats(reset=True)["ungapped_prefilter"]["cells"] > 10000


def _scores_of_many(aln32, targets):
    """the byte loop of `reference` for 250 targets at once in int16 (it holds every value): the rows [column in front of the profile, S(0, j) ..
    S(Lp - 1, j)] of the targets lie end to end, so the step along the diagonals is a shift by one element; what crosses into a row's column 0
    is cleared there, and a step behind a target's end (line 21) clears its whole row"""
    P = np.full((22, len(aln32) + 1), -1000, dtype=np.int16)
    P[:20, 1:], P[20, 1:] = aln32[:, :20].T, 0
    bias = np.int16(abs(min(0, int(P[:20, 1:].min()))))
    P[:21, 1:] += bias                                                                     # the byte of the cell: P[i][a] + bias
    out, order = np.zeros(len(targets), dtype=np.int64), np.argsort([len(t) for t in targets], kind="stable")
    for lo in range(0, len(order), 250):
        idx = order[lo:lo + 250]
        codes = np.full((max(len(targets[k]) for k in idx), len(idx)), 21, dtype=np.int64)
        for r, k in enumerate(idx):
            codes[:len(targets[k]), r] = np.minimum(targets[k], 20)
        prev, cur, best = np.zeros((3, len(idx) * P.shape[1]), dtype=np.int16)
        for row in codes:
            np.add(prev[:-1], P[row].reshape(-1)[1:], out=cur[1:])                         # S(i - 1, j - 1) + byte
            np.minimum(cur, np.int16(255), out=cur)
            cur -= bias
            np.maximum(cur, np.int16(0), out=cur)
            np.maximum(best, cur, out=best)
            prev, cur = cur, prev
        out[idx] = best.reshape(len(idx), -1).max(axis=1)
    return out


def test_golden_profiles_against_the_byte_loop(gpu_api):
    """the 100 golden profiles x the first 2 000 golden fragments: several targets per lane group and band"""
    from test_gpu_profile import _golden_inputs
    api, (_, entries, frags, _, _) = gpu_api, _golden_inputs()
    res, off = api.encode(frags[:2000])
    targets, p = [res[int(off[k]):int(off[k + 1])] for k in range(2000)], _params(api)
    db, q = api.TargetDB.sequences(res, off, p), api.Profiles(entries, p)
    aln = q.derived()[2]
    profs = [aln[int(q.off[i]):int(q.off[i + 1])] for i in range(q.n)]
    hits, hoff = api.ungapped_prefilter(db, q, p)
    want = expected([_scores_of_many(a, targets) for a in profs], profs, targets, np.arange(2000), p)
    assert sum(len(w) for w in want) > 2000 and _lists(hits, hoff, q.n) == want


def test_refusals_by_name(gpu_api, world):
    api, (db, q, _, targets, _, _) = gpu_api, world
    seqs = api.Queries.from_codes(targets[9], _offsets([targets[9]]))
    # a sequence batch against a profile_search database; a profile batch with params.profile_search = 0; the Smith-Waterman filter
    for call, batch, p in ((api.ungapped_prefilter, seqs, _params(api)), (api.ungapped_prefilter, q, api.default_params()), (api.gapped_prefilter, q, _params(api))):
        with pytest.raises(api.MkError, match="error -3.*profile"):
            call(db, batch, p)


def test_commands_ungappedprefilter_align_swapresults(gpu_api, tmp_path):
    from metaeuk_amd import build
    from test_gpu_backtrace import _read_result_db, _write_seq_db
    from test_gpu_profile import GOLD, _golden_inputs
    api, t = gpu_api, str(tmp_path) + "/"
    keys, entries, frags, _, _ = _golden_inputs()
    open(t + "profDB", "wb").write(gzip.open(os.path.join(GOLD, "prof_db.bin.gz"), "rb").read())
    open(t + "profDB.index", "w").write(open(os.path.join(GOLD, "prof_db.index")).read())
    open(t + "profDB.dbtype", "wb").write((2).to_bytes(4, "little"))
    _write_seq_db(t + "aa_6f", frags[:400])
    run = lambda *argv: subprocess.run([build.BIN] + list(argv) + ["--threads", "4"], stderr=subprocess.PIPE, timeout=120)
    r = run("ungappedprefilter", t + "profDB", t + "aa_6f", t + "pref", "--max-seqs", "50")
    assert r.returncode == 0, r.stderr[-300:]
    p, (res, off) = _params(api, max_seqs=50), api.encode(frags[:400])
    q = api.Profiles(entries, p)
    hits, hoff = api.ungapped_prefilter(api.TargetDB.sequences(res, off, p), q, p)
    lists = {keys[i]: api.format_hits(hits, int(hoff[i]), int(hoff[i + 1])) for i in range(q.n)}
    assert _read_result_db(t + "pref") == lists and sum(len(v) for v in lists.values()) > 2000
    assert open(t + "pref.dbtype", "rb").read() == (7).to_bytes(4, "little")
    assert run("align", t + "profDB", t + "aa_6f", t + "pref", t + "aln", "--alignment-mode", "2", "-e", "100").returncode == 0
    assert run("swapresults", t + "profDB", t + "aa_6f", t + "aln", t + "search_res", "-e", "1.79769e+308").returncode == 0
    assert sum(len(v) for v in _read_result_db(t + "search_res").values()) > 200
    r = run("search", t + "aa_6f", t + "profDB", t + "bad", t + "tmp", "--alignment-mode", "2", "--exhaustive-search", "1", "--prefilter-mode", "1")
    assert r.returncode != 0 and b"--prefilter-mode 1" in r.stderr, r.stderr[-300:]
