"""gappedprefilter with profile queries on the GPU (gapped_profile_scores_kernel and the row-tiled kernel's profile image, mk_gapped.hip): every
profile's hit list of mk_gapped_prefilter_profile against the int64 recurrence of test_gapped_profile_host plus the verdict, sort and cut of the
sequence sibling's test, at the shapes where the kernels change path (read from the library); the refusals; the command.  Saturation at 32 767 is
not reachable in the transposed kernel (128 rows x 127 is below it), so no case fakes it; the clamp its cases exercise is the negative one,
H + GAP_PAD in the pad rows and pad columns."""
import ctypes
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

from test_gapped_prefilter_host import evaluer, expected
from test_gapped_profile_host import reference
from test_gpu_gapped_prefilter import _lists
from test_gpu_ungapped_prefilter import _offsets
from test_gpu_ungapped_profile import _params

pytestmark = pytest.mark.gpu


def _make(api, lengths, seed):
    """(db, batch, (aln32 arrays, targets, keys, {1: the score of every pair by the recurrence}, e-value)) -- the world tuple of `expected`"""
    from test_gpu_profile import AA, _synthetic_profile
    rs, rng = np.random.RandomState(seed), random.Random(seed)
    G, rows = api.GAP_GROUP, [api.GAP_ROWS_0, api.GAP_ROWS_1, api.GAP_ROWS_2]
    assert api.GAPP_MAX_TARGET == G * rows[-1]
    rnd = lambda n: rs.randint(0, 20, int(n)).astype(np.uint8)
    entries, cons = zip(*[_synthetic_profile(rng, n) for n in lengths])
    cons = [np.array([AA.index(c) for c in s], dtype=np.uint8) for s in cons]
    # every shape's last full lane, full tile and one beyond (129: the first target of the row-tiled kernel); one target of 300 for its parked row
    targets = [rnd(n) for n in [0, 1] + [G * r + d for r in rows for d in (-1, 0, 1)]] + [np.concatenate([rnd(90), max(cons, key=len)[:160], rnd(50)])]
    for k in range(36):              # pieces of a consensus with point mutations, a deleted and an inserted stretch, inside random flanks
        c = cons[int(rs.randint(min(4, len(cons) - 1), len(cons)))]
        piece = np.array(c[:int(rs.randint(30, 140))])
        piece[rs.rand(len(piece)) < 0.15] = rs.randint(0, 20)
        cut, d = len(piece) // 3, int(rs.randint(2, 5))
        targets.append(np.concatenate([rnd(rs.randint(0, 12)), piece[:cut], piece[cut + d:2 * cut], rnd(d), piece[2 * cut:], rnd(rs.randint(0, 12))]))
    t_off = _offsets(targets)
    assert {int(o) % 4 for o in t_off[:-1]} == {0, 1, 2, 3}                                # target starts on all four bytes of a dword
    db = api.TargetDB.sequences(np.concatenate(targets), t_off, _params(api))
    keys = np.arange(len(targets), dtype=np.uint32)[::-1].copy() * 3 + 5                   # descending: index order is not key order
    assert api.lib().mk_targetdb_set_keys(db.h, keys.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(keys))) == 0
    q = api.Profiles(list(entries), _params(api))
    profs = [q.derived()[2][int(q.off[i]):int(q.off[i + 1])] for i in range(q.n)]
    assert [len(a) for a in profs] == list(lengths)
    return db, q, (profs, targets, keys, {1: [reference(a, targets) for a in profs]}, evaluer(targets))


@pytest.fixture(scope="module")
def world(gpu_api):
    api = gpu_api
    B, W, edge = api.GAPP_BLOCK, api.GAPP_WINDOW, api.GAPP_WINDOW - api.GAPP_LAG
    # one block -1 / 0 / +1; the last profile of one image window, -1 / +1; more than two windows; an odd number: the last register has one half
    db, q, w = _make(api, [1, B - 1, B, B + 1, 64, 150, edge - 1, edge, edge + 1, 2 * W + 37, 90], 37)
    gapless = [[api.ungapped_prefilter_profile_host(a, t) for t in w[1][12:]] for a in w[0][4:]]
    assert q.n % 2 == 1 and sum(int(s) > g for row, grow in zip(w[3][1][4:], gapless) for s, g in zip(row[12:], grow)) > 20      # the gaps pay
    return db, q, w


# name: (parameters, environment); None as a value: an occurring score (the threshold is strict)
VARIANTS = {"defaults": ({}, {}), "cut": (dict(max_seqs=5, min_ungapped_score=0), {}), "threshold": (dict(min_ungapped_score=None), {}),
            "evalue": (dict(evalue_thr=0.001), {}), "filter": (dict(cov_thr=0.8, cov_mode=0), {}),
            "chunks": (dict(max_seqs=7), {"MK_GAPPED_SCORE_BUDGET": str(2 * 2 * 16)}),      # 16 targets x 2 profiles: several chunks both ways
            "rows": ({}, {"MK_GAPPED_PROFILE_ROUTE": "rows"}),                               # every target through the row-tiled kernel
            # a batch that is ONE register pair of 1 and many columns: pad columns in one half for the whole walk of three image windows
            "pair": (dict(min_ungapped_score=3, evalue_thr=1.7976931348623157e308), {})}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_hit_lists_equal_the_recurrence(gpu_api, world, monkeypatch, variant):
    api, (flags, env) = gpu_api, VARIANTS[variant]
    db, q, w = world if variant != "pair" else _make(api, [1, 2 * api.GAPP_WINDOW + 5], 41)
    p = _params(api)
    for k, v in flags.items():
        setattr(p, k, v if v is not None else sorted(int(s) for row in w[3][1] for s in row if s > 15)[40])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    api.kernel_stats(reset=True)
    want, got = expected(w, p), _lists(*api.gapped_prefilter_profile(db, q, p), q.n)
    bad = [(i, len(w[0][i]), got[i][:4], want[i][:4]) for i in range(q.n) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:3])
    assert sum(len(x) for x in want) > {"filter": 3, "evalue": 5, "pair": 7}.get(variant, 20) and all(len(x) > 3 for x in want if variant == "pair")
    if variant == "evalue":                                                                # the default -e keeps more than -e 0.001
        assert sum(len(x) for x in want) < sum(len(x) for x in expected(w, _params(api)))
    assert api.kernel_stats(reset=True)["gapped_prefilter"]["cells"] > 10000


def test_refusals_by_name(gpu_api, world):
    api, (db, q, w) = gpu_api, world
    seqs = api.Queries.from_codes(w[1][9], _offsets([w[1][9]]))
    plain = api.TargetDB.sequences(np.concatenate(w[1]), _offsets(w[1]), api.default_params())
    # a sequence batch; a profile batch with params.profile_search = 0; a database that was not created with profile_search = 1
    for batch, base, p in ((seqs, db, _params(api)), (q, db, api.default_params()), (q, plain, _params(api))):
        with pytest.raises(api.MkError, match="error -3.*profile"):
            api.gapped_prefilter_profile(base, batch, p)


def test_command_gappedprefilter_align_swapresults(gpu_api, tmp_path):
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
    r = run("gappedprefilter", t + "profDB", t + "aa_6f", t + "pref", "--max-seqs", "50")
    assert r.returncode == 0, r.stderr[-300:]
    p, (res, off) = _params(api, max_seqs=50, evalue_thr=0.001), api.encode(frags[:400])  # the module's default -e
    q = api.Profiles(entries, p)
    hits, hoff = api.gapped_prefilter_profile(api.TargetDB.sequences(res, off, p), q, p)
    lists = {keys[i]: api.format_hits(hits, int(hoff[i]), int(hoff[i + 1])) for i in range(q.n)}
    assert _read_result_db(t + "pref") == lists and sum(len(v) for v in lists.values()) > 40
    assert run("align", t + "profDB", t + "aa_6f", t + "pref", t + "aln", "--alignment-mode", "2", "-e", "100").returncode == 0
    assert run("swapresults", t + "profDB", t + "aa_6f", t + "aln", t + "search_res", "-e", "1.79769e+308").returncode == 0
    assert sum(len(v) for v in _read_result_db(t + "search_res").values()) > 40
