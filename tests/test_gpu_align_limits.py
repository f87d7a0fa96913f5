"""--max-accept / --max-rejected on the GPU: the windowed rounds of the alignment stage and its limit-scan kernel (mk_align.hip) against the records
the REAL `metaeuk` binary kept (tests/golden/make_align_limit_golden.sh), byte for byte; hand-made lists that put stops inside, at and across window
boundaries (MK_ALIGN_LIMIT_WINDOW), against the unlimited run of the same lists cut by the rule in Python; the work the stage skips
(mk_align_statistics); the default path, launch for launch; mode 3 / -a; the commands."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from test_align_limits_host import CASES, GOLD, INT_MAX, _blocks, _lines, _text, walk
from test_result_filters_host import can_be_covered

pytestmark = pytest.mark.gpu
L2 = 2097152                                       # tests/golden/PROVENANCE.txt
CASE_PARAMS = {"A": dict(max_accept=1), "B": dict(max_rejected=1), "C": dict(evalue_thr=0.001, max_accept=1, max_rejected=2),
               "D": dict(cov_thr=0.2, cov_mode=5, max_rejected=1)}
CASE_STOPS = {"A": (1276, 0), "B": (0, 492), "C": (322, 237), "D": (0, 1250)}      # tests/golden/PROVENANCE_align_limits.txt
CASE_SCORED = {"A": 4209, "B": 4777, "C": 4209, "D": 3075}


def _params(api, **kw):
    p = api.default_params()
    p.host_l2_bytes = L2
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Ctx:
    pass


def _e2e(api):
    c = Ctx()
    c.api = api
    c.frags = [l.rsplit("\t", 1)[1] for l in _lines("e2e_process_orfs.txt.gz")]
    c.targets = _lines("e2e_targets.txt.gz")
    pref = _blocks(_text("e2e_process_pref.txt.gz"))
    rows = [[tuple(int(x) for x in ln.split("\t")) for ln in pref.get(k, [])] for k in range(len(c.frags))]
    c.off = np.zeros(len(c.frags) + 1, dtype=np.uint64)
    c.off[1:] = np.cumsum([len(r) for r in rows])
    c.hits = np.zeros(int(c.off[-1]), dtype=api.HIT_DTYPE)
    flat = [x for r in rows for x in r]
    c.hits["seq_id"], c.hits["pref_score"], c.hits["diagonal"] = [x[0] for x in flat], [x[1] for x in flat], [x[2] & 0xFFFF for x in flat]
    c.db = api.TargetDB(c.targets, _params(api))
    return c


@pytest.fixture(scope="module")
def e2e(gpu_api):
    return _e2e(gpu_api)


def _formatted(api, result, n):
    alns, aoff = result
    return {i: api.format_alignments(alns, int(aoff[i]), int(aoff[i + 1])).splitlines() for i in range(n) if int(aoff[i + 1]) > int(aoff[i])}


def _same(got, want):
    want = {k: v for k, v in want.items() if v}
    bad = [k for k in set(got) | set(want) if got.get(k, []) != want.get(k, [])]
    assert not bad, (len(bad), sorted(bad)[:5], got.get(bad[0], [])[:3], want.get(bad[0], [])[:3])


def _align_recorded(c, p):
    q = c.api.Queries(c.frags, p)
    c.api.prefilter_result_set(q, c.hits, c.off)
    res = c.api.align(c.db, q, p)
    return q, res


def _check_case(c, case):
    api = c.api
    p = _params(api, **CASE_PARAMS[case])
    q, res = _align_recorded(c, p)
    _same(_formatted(api, res, q.n), _blocks(_text(CASES[case][3])))
    st = api.align_statistics(q)
    print(case, st)
    assert st["pairs_listed"] == 4777 and (st["stopped_accept"], st["stopped_rejected"]) == CASE_STOPS[case]
    # the default schedule (windows of 8, 16, ... pairs) on the recorded lists, derived on the CPU from the rule: the pairs of the windows a walk
    # touches, without the pairs that fail the length test
    assert st["pairs_scored"] == CASE_SCORED[case] and 1 <= st["rounds"] <= 2
    return st


@pytest.mark.parametrize("case", sorted(CASES))
def test_align_on_the_recorded_lists_equals_the_real_process(e2e, case):
    _check_case(e2e, case)


@pytest.mark.parametrize("case", ["A", "B", "C"])        # (case D's --cov-mode 5 also cuts the prefilter's own lists: not the recorded ones)
def test_search_equals_the_real_process(e2e, case):
    api = e2e.api
    p = _params(api, **CASE_PARAMS[case])
    q = api.Queries(e2e.frags, p)
    _, res = api.search(e2e.db, q, p)
    _same(_formatted(api, res, q.n), _blocks(_text(CASES[case][3])))
    st = api.align_statistics(q)
    assert st["pairs_listed"] == 4777 and (st["stopped_accept"], st["stopped_rejected"]) == CASE_STOPS[case]
    # two batches in flight, begun before either is collected
    cut = len(e2e.frags) // 2 + 3
    qs = [api.Queries(e2e.frags[:cut], p), api.Queries(e2e.frags[cut:], p)]
    for x in qs:
        api.search_begin(e2e.db, x, p)
    want = _blocks(_text(CASES[case][3]))
    for k, x in enumerate(qs):
        _, r = api.search_wait(x)
        base = 0 if k == 0 else cut
        _same({base + i: v for i, v in _formatted(api, r, x.n).items()}, {i: v for i, v in want.items() if (i < cut) == (k == 0)})


def _child(code, **env):
    here = os.path.dirname(os.path.abspath(__file__))
    e = dict(os.environ, MK_DEBUG="1", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]), **env)
    r = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def child_host_assembly():
    """(run in a child process: the switch is read once) every golden case and the hand-made lists with the host assembly forced"""
    from metaeuk_amd import api
    api.init(0)
    c = _e2e(api)
    for case in sorted(CASES):
        _check_case(c, case)
    s = _synth(api)
    os.environ["MK_ALIGN_LIMIT_WINDOW"] = "3"
    _check_lists(s, 3, filtered=False)
    _check_lists(s, 3, filtered=True)
    print("host assembly: ok")


def test_host_assembly_decides_with_the_twin():
    out = _child("import test_gpu_align_limits as t; t.child_host_assembly()", MK_ALIGN_HOST_ASSEMBLE="1")
    assert "host assembly: ok" in out


# ---- hand-made lists on a synthetic set ------------------------------------------------------------------------------------------------
EVALUE = 1e-3
LIMITS = [(1, INT_MAX), (2, INT_MAX), (INT_MAX, 1), (INT_MAX, 3), (2, 2), (3, 5), (4, 66), (INT_MAX, 0), (5, 0)]


def _synth(api):
    """40 fragments x 300 proteins (families of 10: a fragment's family are its homologs, accepted at -e 0.001; other proteins are rejected)"""
    s = Ctx()
    s.api = api
    s.t_res, s.t_off = api.synth_targets(300, seed=23)
    s.f_res, s.f_off, s.src = api.synth_fragments(40, s.t_res, s.t_off, seed=23, mutation_rate=0.1, min_len=40, max_len=80)
    s.db = api.TargetDB.from_codes(s.t_res, s.t_off, _params(api))
    rs = np.random.RandomState(23)
    lists = []
    for i in range(40):
        fam = [int(s.src[i]) // 10 * 10 + j for j in range(10)]
        rs.shuffle(fam)
        other = [int(t) for t in rs.permutation(300) if int(t) // 10 != int(s.src[i]) // 10]
        H, R = (lambda k: [fam.pop() for _ in range(k)]), (lambda k: [other.pop() for _ in range(k)])
        shapes = [
            lambda: [],    # 0 pairs
            lambda: H(1), lambda: R(1),    # 1 pair
            lambda: R(2) + H(1), lambda: R(3),    # exactly a window of 3: an accept / the third rejection on its last pair
            lambda: R(3) + H(1), lambda: R(2) + H(1) + R(1),    # window + 1
            lambda: H(1) + R(2) + H(1) + R(2) + H(1) + R(2) + H(1) + R(5),    # several windows, every accept on a window's first pair
            lambda: R(2) + H(2) + R(1) + H(1) + R(4) + H(1),    # a streak that spans two windows (pairs 2 / 3 and 5 / 6 lie in different windows of 3)
            lambda: R(1) + H(1) + R(1) + H(1) + R(1) + H(1) + R(1) + H(1),    # the accept limit falls in the middle of a window
            lambda: H(3),    # the list ends before any stop
            lambda: R(66) + H(2) + R(3) + H(1),    # more than 64 pairs: a long streak, then accepts in the second step of the scan
            lambda: R(30) + H(1) + R(40) + H(2),
            lambda: H(2) + R(63) + H(1) + R(4) + H(3),
        ]
        lists.append(shapes[i]() if i < len(shapes) else [x for _ in range(int(rs.randint(1, 9))) for x in (R(int(rs.randint(0, 6))) + H(int(rs.randint(0, 2))))])
    s.lists = lists
    s.off = np.zeros(41, dtype=np.uint64)
    s.off[1:] = np.cumsum([len(l) for l in lists])
    s.hits = np.zeros(int(s.off[-1]), dtype=api.HIT_DTYPE)
    s.hits["seq_id"] = [t for l in lists for t in l]
    s.q_len = np.diff(s.f_off).astype(int)
    s.t_len = np.diff(s.t_off).astype(int)
    return s


@pytest.fixture(scope="module")
def synth(gpu_api):
    return _synth(gpu_api)


def _run_lists(s, p):
    q = s.api.Queries.from_codes(s.f_res, s.f_off, p)
    s.api.prefilter_result_set(q, s.hits, s.off)
    alns, aoff = s.api.align(s.db, q, p)
    got = [[(int(alns[k].db_key), s.api.format_alignments(alns, k, k + 1)) for k in range(int(aoff[i]), int(aoff[i + 1]))] for i in range(40)]
    return got, s.api.align_statistics(q)


def _check_lists(s, window, filtered):
    """every limit pair against the unlimited run of the same lists cut by the rule; window = the fixed window in force (None: the default schedule)"""
    flt = dict(cov_thr=0.15, cov_mode=5) if filtered else {}
    base, st0 = _run_lists(s, _params(s.api, evalue_thr=EVALUE, **flt))
    n_pairs = int(s.off[-1])
    cut = [[filtered and not can_be_covered(0.15, 5, s.q_len[i], s.t_len[t]) for t in l] for i, l in enumerate(s.lists)]
    n_cut = sum(sum(c) for c in cut)
    assert st0 == dict(pairs_listed=n_pairs, pairs_scored=n_pairs - n_cut, stopped_accept=0, stopped_rejected=0, rounds=1)
    assert not filtered or n_cut >= 10
    n_acc = sum(len(b) for b in base)
    assert 25 <= n_acc <= n_pairs - 100                          # planted homologs accepted, unrelated pairs rejected
    seen = set()
    for a, r in LIMITS:
        got, st = _run_lists(s, _params(s.api, evalue_thr=EVALUE, max_accept=a, max_rejected=r, **flt))
        bound = stops_a = stops_r = 0
        for i, l in enumerate(s.lists):
            acc = {t: line for t, line in base[i]}
            verdicts = [2 if c else (1 if t in acc else 0) for t, c in zip(l, cut[i])]
            keep, looked, state = walk(verdicts, a, r)
            want = [acc[t] for t, k in zip(l, keep) if k]
            assert sorted(x[1] for x in got[i]) == sorted(want), (window, filtered, a, r, i, l, verdicts)
            # the kept records in the order of the unlimited run (Matcher::compareHits does not look at the other records)
            order = [line for _, line in base[i]]
            assert [x[1] for x in got[i]] == [ln for ln in order if ln in set(want)], (window, a, r, i)
            stops_a += state[2] == 1; stops_r += state[2] == 2
            if window:
                reach = min(len(l), -(-looked // window) * window)
                bound += sum(1 for c in cut[i][:reach] if not c)
                if state[2] and looked < len(l):
                    seen.add("last pair of a window" if looked % window == 0 else "inside a window")
                if state[2] and looked > window:
                    seen.add("behind the first window")
                if len(l) > 64 and 64 < looked:
                    seen.add("beyond 64 pairs")
        assert (st["stopped_accept"], st["stopped_rejected"], st["pairs_listed"]) == (stops_a, stops_r, n_pairs), (a, r, st)
        if window:
            assert st["pairs_scored"] <= bound, (window, a, r, st, bound)
        if (a, r) in ((1, INT_MAX), (INT_MAX, 1), (2, 2)):
            assert st["pairs_scored"] < st0["pairs_scored"] and st["rounds"] >= 1, (window, a, r, st, st0)
    if window in (1, 3):
        assert seen == {"last pair of a window", "inside a window", "behind the first window", "beyond 64 pairs"} - ({"inside a window"} if window == 1 else set()), seen


@pytest.mark.parametrize("window,filtered", [(1, False), (3, False), (3, True), (None, False), (None, True)])
def test_hand_made_lists_under_every_window(synth, monkeypatch, window, filtered):
    if window:
        monkeypatch.setenv("MK_ALIGN_LIMIT_WINDOW", str(window))           # (read per call, under MK_DEBUG=1)
    else:
        monkeypatch.delenv("MK_ALIGN_LIMIT_WINDOW", raising=False)
    _check_lists(synth, window, filtered)


# ---- the default path ---------------------------------------------------------------------------------------------------------------------
def test_default_limits_run_the_same_launches(e2e):
    api = e2e.api
    runs = []
    for kw in ({}, dict(max_accept=INT_MAX, max_rejected=INT_MAX), dict(max_accept=0, max_rejected=0)):
        p = _params(api, **kw)
        api.kernel_stats(reset=True)
        q, res = _align_recorded(e2e, p)
        st = api.kernel_stats(reset=True)
        runs.append({k: v["launches"] for k, v in st.items() if not k.startswith("host_") and not k.startswith("wait_")})
        _same(_formatted(api, res, q.n), _blocks(_text("e2e_process_aln.txt.gz")))
        assert not [k for k in st if "limit" in k], sorted(st)
        assert api.align_statistics(q) == dict(pairs_listed=4777, pairs_scored=4777, stopped_accept=0, stopped_rejected=0, rounds=1)
    assert runs[0] == runs[1] == runs[2] and sum(runs[0].values()) > 10, runs
    api.kernel_stats(reset=True)
    _align_recorded(e2e, _params(api, max_accept=1))
    assert api.kernel_stats(reset=True)["align_limit_scan"]["launches"] >= 1


# ---- mode 3 / -a ------------------------------------------------------------------------------------------------------------------------------
def test_mode3_with_backtraces_equals_the_real_process(e2e):
    api = e2e.api
    p = _params(api, alignment_mode=3, add_backtrace=1, max_accept=2, max_rejected=2, evalue_thr=0.001)
    want = _blocks(_text("e2e_limit_search_res_m3a.txt.gz"))
    for how in ("search", "align"):
        q = api.Queries(e2e.frags, p)
        if how == "search":
            _, (alns, aoff) = api.search(e2e.db, q, p)
        else:
            api.prefilter_result_set(q, e2e.hits, e2e.off)
            alns, aoff = api.align(e2e.db, q, p)
        n = int(aoff[-1])
        assert n == 640                                           # tests/golden/PROVENANCE_align_limits.txt
        ops, ooff, ids = api.align_backtrace(q, n)
        assert api.trace_left_band(q) == 0 and len(ooff) == n + 1
        got = {i: api.format_alignments_bt_bulk(alns, int(aoff[i]), int(aoff[i + 1]), ops, ooff).decode().splitlines()
               for i in range(q.n) if int(aoff[i + 1]) > int(aoff[i])}
        _same(got, want)


def test_profiles_and_negative_limits_are_refused(e2e):
    api = e2e.api
    q = api.Queries(e2e.frags[:50], _params(api))
    for kw in (dict(max_accept=-1), dict(max_rejected=-7)):
        with pytest.raises(api.MkError, match="error -1"):
            api.search(e2e.db, q, _params(api, **kw))
    for kw in (dict(max_accept=1), dict(max_rejected=3)):
        with pytest.raises(api.MkError, match="error -3") as e:
            api.search(e2e.db, q, _params(api, profile_search=1, **kw))
        assert "--max-accept" in str(e.value) and "profile" in str(e.value)


# ---- the commands, from DBs on disk -----------------------------------------------------------------------------------------------------
def _write_seq_db(base, seqs, dbtype=0):
    off = 0
    with open(base, "wb") as d, open(base + ".index", "w") as i:
        for k, s in enumerate(seqs):
            d.write(s.encode() + b"\n\0")
            i.write("%d\t%d\t%d\n" % (k, off, len(s) + 2))
            off += len(s) + 2
    with open(base + ".dbtype", "wb") as t:
        t.write(int(dbtype).to_bytes(4, "little"))


def _read_result_db(base):
    data = open(base, "rb").read()
    out = {}
    for line in open(base + ".index"):
        k, o, l = line.split("\t")
        out[int(k)] = data[int(o):int(o) + int(l) - 1].decode()
    return out


def test_commands_equal_the_real_process(e2e, tmp_path):
    from metaeuk_amd import build
    t = str(tmp_path) + "/"
    _write_seq_db(t + "targets", e2e.targets)
    _write_seq_db(t + "contigs", _lines("e2e_contigs.txt.gz"), 1)
    _write_seq_db(t + "aa_6f", e2e.frags)
    pref = _blocks(_text("e2e_process_pref.txt.gz"))
    off = 0
    with open(t + "pref_0", "wb") as d, open(t + "pref_0.index", "w") as i:
        for k in range(len(e2e.frags)):
            body = "".join(ln + "\n" for ln in pref.get(k, [])).encode() + b"\0"
            d.write(body); i.write("%d\t%d\t%d\n" % (k, off, len(body))); off += len(body)
    open(t + "pref_0.dbtype", "wb").write((7).to_bytes(4, "little"))
    blocks = lambda d: "".join(">%d\n%s" % (k, d[k]) for k in sorted(d))
    common = ["--alignment-mode", "2", "--min-aln-len", "11", "--threads", "4", "--ref-l2-bytes", str(L2)]
    flags = {"A": ["-e", "100", "--max-accept", "1"], "B": ["-e", "100", "--max-rejected", "1"], "C": ["-e", "0.001", "--max-accept", "1", "--max-rejected", "2"],
             "D": ["-e", "100", "-c", "0.2", "--cov-mode", "5", "--max-rejected", "1"]}
    for case in sorted(flags):
        subprocess.check_call([build.BIN, "align", t + "aa_6f", t + "targets", t + "pref_0", t + "res" + case] + common + flags[case], stderr=subprocess.DEVNULL)
        assert blocks(_read_result_db(t + "res" + case)) == _text(CASES[case][3]), case
    subprocess.check_call([build.BIN, "search", t + "aa_6f", t + "targets", t + "res_search", t + "tmp", "-s", "5.7"] + common + flags["C"], stderr=subprocess.DEVNULL)
    assert blocks(_read_result_db(t + "res_search")) == _text("e2e_limit_aln_C.txt.gz")
    pe = ["--threads", "4", "--ref-l2-bytes", str(L2), "-s", "5.7"]
    subprocess.check_call([build.BIN, "predictexons", t + "contigs", t + "targets", t + "calls1", t + "tmp", "--max-accept", "1"] + pe, stderr=subprocess.DEVNULL)
    assert blocks(_read_result_db(t + "calls1")) == _text("e2e_limit_calls_acc1.txt.gz")
    subprocess.check_call([build.BIN, "predictexons", t + "contigs", t + "targets", t + "calls2", t + "tmp", "--alignment-mode", "3", "-a", "1", "--max-accept", "2",
                           "--max-rejected", "2", "-e", "0.001"] + pe, stderr=subprocess.DEVNULL)
    assert blocks(_read_result_db(t + "calls2")) == _text("e2e_limit_calls_m3a.txt.gz")
    assert _text("e2e_limit_calls_acc1.txt.gz") != _text("e2e_exons_expected.txt.gz")
    # values the reference's pattern ^[1-9][0-9]*$ does not admit: refused by name, nothing written
    for bad in (["--max-accept", "0"], ["--max-rejected", "x"], ["--max-accept", "-3"], ["--max-rejected", "99999999999"]):
        r = subprocess.run([build.BIN, "align", t + "aa_6f", t + "targets", t + "pref_0", t + "res_bad"] + common + bad, capture_output=True)
        assert r.returncode != 0 and bad[0].encode() in r.stderr, (bad, r.stderr[-300:])
        assert not os.path.exists(t + "res_bad.dbtype")
    # a profile target database: the reference aligns twice there, the limits are refused by name
    (tmp_path / "profDB").write_bytes(gzip.open(os.path.join(GOLD, "prof_db.bin.gz"), "rb").read())
    (tmp_path / "profDB.index").write_text(open(os.path.join(GOLD, "prof_db.index")).read())
    (tmp_path / "profDB.dbtype").write_bytes((2).to_bytes(4, "little"))
    for bad in (["--max-accept", "1"], ["--max-rejected", "2"]):
        r = subprocess.run([build.BIN, "predictexons", t + "contigs", t + "profDB", t + "calls_bad", t + "tmp"] + pe + bad, capture_output=True)
        assert r.returncode != 0 and bad[0].encode() in r.stderr and b"profile" in r.stderr, (bad, r.stderr[-300:])
        assert not os.path.exists(t + "calls_bad.dbtype")
