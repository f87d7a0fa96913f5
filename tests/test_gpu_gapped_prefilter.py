"""gappedprefilter on the GPU: every query's hit list of mk_gapped_prefilter (mk_gapped.hip) against the list built from oracle.sw scores plus the verdict,
sort and cut of test_gapped_prefilter_host.expected, at the shapes where the kernel changes path (read from the library); the command against the call."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

import oracle
from test_gapped_prefilter_host import build_world, evaluer, expected, golden_saturating_pair, rnd

pytestmark = pytest.mark.gpu


def _db(api, targets, keys):
    db = api.TargetDB.sequences(*api.encode(targets))
    assert api.lib().mk_targetdb_set_keys(db.h, keys.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(len(keys))) == 0
    return db


def _lists(hits, off, n):
    return [[(int(h["seq_id"]), int(h["pref_score"])) for h in hits[int(off[i]):int(off[i + 1])]] for i in range(n)]


@pytest.fixture(scope="module")
def world(gpu_api):
    w = build_world()
    return w, _db(gpu_api, w[1], w[2]), gpu_api.Queries(w[0])


# name: (parameters, score budget in bytes or None); None as a value: an occurring score (the threshold is strict)
VARIANTS = {"defaults": ({}, None), "no bias": (dict(comp_bias_corr=0), None), "cut": (dict(max_seqs=5, min_ungapped_score=0), None),
            "threshold": (dict(min_ungapped_score=None), None), "filter": (dict(cov_thr=0.8, cov_mode=0), None),
            "evalue": (dict(evalue_thr=0.001), None), "chunks": (dict(max_seqs=7), 2 * 2 * 16)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_hit_lists_equal_the_oracle(gpu_api, world, monkeypatch, variant):
    api, (w, db, q) = gpu_api, world
    flags, budget = VARIANTS[variant]
    p = api.default_params()
    for k, v in flags.items():
        setattr(p, k, v if v is not None else sorted(s for row in w[3][1] for s in row if s > 15)[40])
    if budget:
        monkeypatch.setenv("MK_GAPPED_SCORE_BUDGET", str(budget))                          # 16 targets x 2 queries: several chunks both ways
    api.kernel_stats(reset=True)
    want = expected(w, p, 1 if p.comp_bias_corr else 0)
    hits, off = api.gapped_prefilter(db, q, p)
    got = _lists(hits, off, len(w[0]))
    bad = [(i, len(w[0][i]), got[i][:4], want[i][:4]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:3])
    assert all(int(h["diagonal"]) == 0 for h in hits) and sum(len(x) for x in want) > {"filter": 3, "evalue": 5}.get(variant, 20)
    if variant == "evalue":                                                                # -e 100 keeps more than -e 0.001
        assert sum(len(x) for x in want) < sum(len(x) for x in expected(w, api.default_params()))
    assert api.kernel_stats(reset=True)["gapped_prefilter"]["cells"] > 10000


def test_one_packed_pair_of_lengths_1_and_64(gpu_api, world):
    """a batch that is ONE register pair: 63 pad rows beside real ones"""
    api, (w, db, _) = gpu_api, world
    queries = ["W", w[0][8]]
    assert len(queries[1]) == 64
    scores = {1: [[oracle.sw(q, t, with_start=False)[0] for t in w[1]] for q in queries]}
    p = api.default_params()
    p.min_ungapped_score, p.evalue_thr = 3, sys.float_info.max                            # no e-value test: the 1-residue query keeps its identities
    want = expected((queries, w[1], w[2], scores, w[4]), p)
    assert _lists(*api.gapped_prefilter(db, api.Queries(queries), p), 2) == want and all(len(x) > 3 for x in want)


def test_saturating_pair_scores_32767(gpu_api):
    """the sw2_* golden's saturating pair and one neighbour, 2 x 3: row tiles, the parked row, the clamped add"""
    api, rs = gpu_api, np.random.RandomState(3)
    q, t = golden_saturating_pair()
    queries, targets = [q, q[100:140]], [rnd(rs, 50), t, q[90:150]]
    keys = np.array([9, 5, 7], dtype=np.uint32)
    scores = {1: [[oracle.sw(a, b, with_start=False)[0] for b in targets] for a in queries]}
    want = expected((queries, targets, keys, scores, evaluer(targets)), api.default_params())
    assert want[0][0] == (1, 32767) and len(want[1]) >= 1
    assert _lists(*api.gapped_prefilter(_db(api, targets, keys), api.Queries(queries)), 2) == want


def test_command_equals_the_call_and_refusals_by_name(gpu_api, world, tmp_path):
    from metaeuk_amd import build
    from test_backtrace_host import _lines
    from test_gpu_backtrace import _read_result_db, _write_seq_db
    from test_gpu_profile import _golden_inputs
    api, t = gpu_api, str(tmp_path) + "/"
    with pytest.raises(api.MkError, match="error -3.*profile"):
        api.gapped_prefilter(world[1], api.Profiles(_golden_inputs()[1][:1]))
    frags, targets = [l.rsplit("\t", 1)[1] for l in _lines("e2e_process_orfs.txt.gz")][:400], _lines("e2e_targets.txt.gz")
    _write_seq_db(t + "targets", targets); _write_seq_db(t + "aa_6f", frags)
    run = lambda *argv: subprocess.run([build.BIN] + list(argv), stderr=subprocess.PIPE, timeout=120)
    assert run("gappedprefilter", t + "aa_6f", t + "targets", t + "pref", "--max-seqs", "20", "--threads", "4").returncode == 0
    assert open(t + "pref.dbtype", "rb").read() == (7).to_bytes(4, "little")
    p = api.default_params()
    p.max_seqs, p.evalue_thr = 20, 0.001                                                   # the module's default -e
    hits, off = api.gapped_prefilter(api.TargetDB.sequences(*api.encode(targets)), api.Queries(frags), p)
    got = _read_result_db(t + "pref")
    assert len(hits) > 40 and all(got[i] == api.format_hits(hits, int(off[i]), int(off[i + 1])) for i in range(len(frags)))
    assert run("align", t + "aa_6f", t + "targets", t + "pref", t + "aln", "--alignment-mode", "2", "--threads", "4").returncode == 0
    assert len(open(t + "aln", "rb").read()) > 1000
    for bad in (["gappedprefilter", t + "aa_6f", t + "targets", t + "bad", "--taxon-list", "9606"], ["gappedprefilter", t + "aa_6f", t + "aa_6f", t + "bad"]):
        r = run(*bad)
        assert r.returncode != 0 and (b"--taxon-list" in r.stderr or b"query DB as the target DB" in r.stderr), (bad, r.stderr[-300:])
