"""--alignment-mode 3 / -a on the GPU: the backtrace kernel (mk_trace.hip) against its host twin (mk_backtrace_host) on explicit pairs, and the
search path against the records the REAL `metaeuk` binary wrote with `--alignment-mode 3 -a 1` (tests/golden/make_backtrace_golden.sh),
byte for byte.  Every test asserts that no trace left the band on its inputs."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import oracle
from test_backtrace_host import _blocks, _lines, _text, compress
from test_result_filters_host import can_be_covered, has_coverage

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
L2 = 2097152                                       # tests/golden/PROVENANCE.txt


def _mat():
    m = oracle.submat(0, 2.0, 0.0)
    return np.array([[m.sub[i][j] for j in range(21)] for i in range(21)], dtype=np.int8)


def _params(api, mode=0, a=0, sid_mode=0, **kw):
    p = api.default_params()
    p.host_l2_bytes = L2
    p.alignment_mode, p.add_backtrace, p.seq_id_mode = mode, a, sid_mode
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _twin_check(api, db, q, q_res, q_off, t_res, t_off, q_idx, t_idx):
    """mk_sw_pairs(with_start) + mk_sw_backtrace_pairs against mk_backtrace_host on the same rectangles -> (in5, strings, attempts, bands)"""
    in5 = api.sw_pairs(db, q, q_idx, t_idx, with_start=True)
    strings, bt, ids, att, band = api.sw_backtrace_pairs(db, q, q_idx, t_idx, in5)
    _, _, bias8 = q.derived()
    mat = _mat()
    bad = []
    for p in range(len(q_idx)):
        score, qe, te, qs, ts = (int(x) for x in in5[p])
        if score <= 0:
            assert (int(bt[p]), int(ids[p]), int(att[p])) == (0, 0, 0)
            continue
        qo, to = int(q_off[q_idx[p]]), int(t_off[t_idx[p]])
        ops, hids, hatt = api.backtrace_host(mat, q_res[qo + qs:qo + qe + 1], bias8[qo + qs:qo + qe + 1], t_res[to + ts:to + te + 1], score)
        assert ops is not None, ("the trace left the band", p)
        if (strings[p], int(bt[p]), int(ids[p]), int(att[p])) != (ops, len(ops), hids, hatt):
            bad.append((p, strings[p], ops, int(ids[p]), hids, int(att[p]), hatt))
        assert int(band[p]) == (abs((te - ts) - (qe - qs)) + 1) << (hatt - 1)
    assert not bad, (len(bad), bad[:2])
    return in5, strings, att, band


def test_kernel_equals_host_twin_on_the_corner_fixture(gpu_api):
    api = gpu_api
    queries, targets = _lines("bt_corner_queries.txt.gz"), _lines("bt_corner_targets.txt.gz")
    recs = [(qk, ln.split("\t")) for qk, lines in sorted(_blocks(_text("bt_corner_aln.txt.gz")).items()) for ln in lines]
    q_idx = np.array([r[0] for r in recs], dtype=np.uint32)
    t_idx = np.array([int(r[1][0]) for r in recs], dtype=np.uint32)
    p = _params(api)
    db, q = api.TargetDB(targets, p), api.Queries(queries, p)
    api.kernel_stats(reset=True)
    in5, strings, att, band = _twin_check(api, db, q, q.res, q.off, db.res, db.off, q_idx, t_idx)
    st = api.kernel_stats(reset=True)
    # ... and the reference's own records: coordinates and the compressed string of column 11
    for k, (qk, c) in enumerate(recs):
        assert [int(in5[k][3]), int(in5[k][1]), int(in5[k][4]), int(in5[k][2])] == [int(c[4]), int(c[5]), int(c[7]), int(c[8])]
        assert compress(strings[k].decode()) == c[10], (qk, c)
    # the classes up to a band of 128 were reached: 11 ints per LDS row (band <= 4), 23 (<= 10), 67 (<= 32), 259 (<= 128); the wider ones: the next test
    assert int(att.max()) >= 7 and int(band.min()) <= 4
    for lo, hi in ((4, 10), (10, 32), (32, 128)):
        assert any(lo < int(b) <= hi for b in band), (lo, hi)
    for name in ("sw_trace_lds11", "sw_trace_lds23", "sw_trace_lds67", "sw_trace_lds259"):
        assert st[name]["launches"] >= 1 and st[name]["cells"] > 0, (name, sorted(st))


def test_kernel_equals_host_twin_on_random_pairs(gpu_api):
    """2 000 planted fragments against their source proteins, 500 of them against an unrelated protein as well, and the shortest rectangles:
    fragments of 1, 2 and 11 residues (a one-cell rectangle gives 1M)"""
    api = gpu_api
    t_res, t_off = api.synth_targets(300, seed=5)
    f_res, f_off, src = api.synth_fragments(2000, t_res, t_off, seed=5, mutation_rate=0.15, min_len=20, max_len=80)
    rs = np.random.RandomState(5)
    extra, extra_src = [], []
    for n in (1, 2, 11):
        for t in (0, 7, 19):
            lo = int(t_off[t]) + 30
            extra.append(np.array(t_res[lo:lo + n])); extra_src.append(t)
    for t in (3, 4, 5, 6):                          # ... and fragments that lost two residues in the middle, or gained three
        lo = int(t_off[t]) + 20
        seg = np.array(t_res[lo:lo + 70])
        extra.append(np.concatenate([seg[:30], seg[32:]])); extra_src.append(t)
        extra.append(np.concatenate([seg[:40], seg[10:13], seg[40:]])); extra_src.append(t)
    # ... one whose band (first band 701) is beyond the classes that keep their rows in LDS: the two halves of a fragment lie 700 residues apart;
    # and one with 300 residues between its halves (first band 301: the widest LDS class)
    long_t = rs.randint(0, 20, 1600).astype(np.uint8)
    t_res = np.concatenate([t_res[:int(t_off[-1])], long_t]); t_off = np.concatenate([t_off, [int(t_off[-1]) + 1600]]).astype(np.uint64)
    extra.append(np.concatenate([long_t[100:450], long_t[1150:1500]])); extra_src.append(300)
    extra.append(np.concatenate([long_t[100:300], long_t[600:800]])); extra_src.append(300)
    q_res = np.concatenate([f_res[:int(f_off[-1])]] + extra).astype(np.uint8)
    q_off = np.concatenate([f_off, int(f_off[-1]) + np.cumsum([len(e) for e in extra])]).astype(np.uint64)
    src = np.concatenate([src, np.array(extra_src, dtype=np.uint32)])
    nq = len(q_off) - 1
    q_idx = np.concatenate([np.arange(nq), np.arange(500)]).astype(np.uint32)
    t_idx = np.concatenate([src, rs.randint(0, 300, 500)]).astype(np.uint32)
    p = _params(api)
    db, q = api.TargetDB.from_codes(t_res, t_off, p), api.Queries.from_codes(q_res, q_off, p)
    api.kernel_stats(reset=True)
    in5, strings, att, band = _twin_check(api, db, q, q_res, q_off, t_res, t_off, q_idx, t_idx)
    one = [k for k in range(2000, 2003)]
    assert all(int(in5[k][0]) > 0 and strings[k] == b"M" for k in one), [(in5[k], strings[k]) for k in one]
    assert all(len(strings[k]) == 2 for k in range(2003, 2006)) and all(len(strings[k]) == 11 for k in range(2006, 2009))
    assert sum(1 for s in strings[2009:2017] if b"I" in s or b"D" in s) >= 6
    assert int(att.max()) >= 2
    st = api.kernel_stats(reset=True)
    assert strings[2017].count(b"D") >= 650 and int(band[2017]) >= 701 and st["sw_trace_global"]["launches"] >= 1
    assert strings[2018].count(b"D") >= 280 and 128 < int(band[2018]) <= 512 and st["sw_trace_lds1027"]["launches"] >= 1


# ---- end to end: the e2e fixture in mode 3 with -a ------------------------------------------------------------------------------------
class E2E:
    pass


@pytest.fixture(scope="module")
def e2e(gpu_api):
    c = E2E()
    c.api = gpu_api
    c.frags = [l.rsplit("\t", 1)[1] for l in _lines("e2e_process_orfs.txt.gz")]
    c.targets = _lines("e2e_targets.txt.gz")
    c.want = _blocks(_text("e2e_process_aln_m3a.txt.gz"))
    c.db = gpu_api.TargetDB(c.targets, _params(gpu_api))
    return c


def _formatted_bt(api, q, result, key0=0):
    """{query key: [11-column lines]} of a batch searched with -a"""
    alns, aoff = result
    n = int(aoff[-1])
    ops, ooff, ids = api.align_backtrace(q, n)
    assert api.trace_left_band(q) == 0
    assert all(int(ooff[k + 1]) > int(ooff[k]) for k in range(n))                       # a path for every record
    out = {}
    for i in range(q.n):
        body = api.format_alignments_bt_bulk(alns, int(aoff[i]), int(aoff[i + 1]), ops, ooff).decode()
        out[key0 + i] = body.splitlines()
    return out


def _same(got, want):
    bad = [k for k in got if got[k] != want.get(k, [])]
    assert not bad, (len(bad), bad[:5], got[bad[0]][:2], want.get(bad[0], [])[:2])
    assert sum(len(v) for v in got.values()) == sum(len(want.get(k, [])) for k in got)


def test_search_equals_the_real_process(e2e):
    api = e2e.api
    p = _params(api, 3, 1)
    q = api.Queries(e2e.frags, p)
    api.kernel_stats(reset=True)
    _, res = api.search(e2e.db, q, p)
    st = api.kernel_stats(reset=True)
    got = _formatted_bt(api, q, res)
    _same(got, e2e.want)
    assert sum(len(v) for v in got.values()) == 4169
    assert sum(v["cells"] for k, v in st.items() if k.startswith("sw_trace")) > 0
    e2e.trace_cells = sum(v["cells"] for k, v in st.items() if k.startswith("sw_trace"))
    # ... the same through mk_prefilter + mk_align, and a second time: identical bytes
    q2 = api.Queries(e2e.frags, p)
    api.prefilter(e2e.db, q2, p)
    assert _formatted_bt(api, q2, api.align(e2e.db, q2, p)) == got
    q3 = api.Queries(e2e.frags, p)
    _, res3 = api.search(e2e.db, q3, p)
    assert _formatted_bt(api, q3, res3) == got
    # mode 3 without -a: the same ten columns, no strings kept
    p3 = _params(api, 3, 0)
    q4 = api.Queries(e2e.frags, p3)
    _, (alns, aoff) = api.search(e2e.db, q4, p3)
    ten = {i: api.format_alignments(alns, int(aoff[i]), int(aoff[i + 1])).splitlines() for i in range(q4.n)}
    assert ten == {k: [ln.rsplit("\t", 1)[0] for ln in v] for k, v in got.items()}
    with pytest.raises(api.MkError, match="error -1"):
        api.align_backtrace(q4, int(aoff[-1]))


def test_three_batches_in_flight_keep_their_own_strings(e2e):
    api = e2e.api
    p = _params(api, 3, 1)
    n = len(e2e.frags)
    cuts = [0, n // 3, 2 * n // 3 + 7, n]
    qs = [api.Queries(e2e.frags[cuts[k]:cuts[k + 1]], p) for k in range(3)]
    for q in qs:
        api.search_begin(e2e.db, q, p)
    for k, q in enumerate(qs):
        _, res = api.search_wait(q)
        got = _formatted_bt(api, q, res, cuts[k])
        assert sum(len(v) for v in got.values()) > 500
        _same(got, e2e.want)


def test_min_seq_id_and_seq_id_mode(e2e):
    api = e2e.api
    p = _params(api, 3, 1, 1, seq_id_thr=0.3)
    q = api.Queries(e2e.frags, p)
    _, res = api.search(e2e.db, q, p)
    want = _blocks(_text("e2e_process_aln_m3a_id03.txt.gz"))
    got = _formatted_bt(api, q, res)
    _same(got, want)
    assert 100 <= sum(len(v) for v in got.values()) <= 4169 - 100


def test_coverage_filter_drops_the_trace_jobs(e2e):
    """-c 0.8 --cov-mode 2: the records whose query coverage misses the threshold get no trace job (StripedSmithWaterman.cpp:485-489) -- fewer
    band cells in the trace kernels than the unfiltered run's, the kept records those of the unfiltered fixture"""
    api = e2e.api
    thr, mode = 0.8, 2

    def passes(ln):
        c = ln.split("\t")
        qs, qe, ql, ts, te, tl = (int(x) for x in c[4:10])
        return can_be_covered(thr, mode, ql, tl) and has_coverage(thr, mode, F(qe - qs + 1) / F(ql), F(te - ts + 1) / F(tl))
    want = {k: [ln for ln in v if passes(ln)] for k, v in e2e.want.items()}
    kept = sum(len(v) for v in want.values())
    assert 100 <= kept <= 4169 - 100
    p = _params(api, 3, 1, cov_thr=thr, cov_mode=mode)
    q = api.Queries(e2e.frags, p)
    api.kernel_stats(reset=True)
    _, res = api.search(e2e.db, q, p)
    st = api.kernel_stats(reset=True)
    _same(_formatted_bt(api, q, res), want)
    cells = sum(v["cells"] for k, v in st.items() if k.startswith("sw_trace"))
    if not hasattr(e2e, "trace_cells"):
        pu = _params(api, 3, 1)
        qu = api.Queries(e2e.frags, pu)
        api.search(e2e.db, qu, pu)
        e2e.trace_cells = sum(v["cells"] for k, v in api.kernel_stats(reset=True).items() if k.startswith("sw_trace"))
    print("trace cells: %.0f unfiltered, %.0f with -c 0.8 --cov-mode 2 (%d of 4169 records kept)" % (e2e.trace_cells, cells, kept))
    assert 0 < cells < e2e.trace_cells


def test_default_mode_is_unchanged(e2e):
    api = e2e.api
    for p in (_params(api), _params(api, 2, 0, 2)):
        q = api.Queries(e2e.frags, p)
        api.kernel_stats(reset=True)
        _, (alns, aoff) = api.search(e2e.db, q, p)
        st = api.kernel_stats(reset=True)
        want = _blocks(_text("e2e_process_aln.txt.gz"))
        got = {i: api.format_alignments(alns, int(aoff[i]), int(aoff[i + 1])).splitlines() for i in range(q.n)}
        _same(got, want)
        assert not [k for k in st if "trace" in k], sorted(st)
        with pytest.raises(api.MkError, match="error -1"):
            api.align_backtrace(q, int(aoff[-1]))


def test_arguments_and_profiles(e2e):
    api = e2e.api
    q = api.Queries(e2e.frags[:50], _params(api))
    for kw, code in ((dict(mode=1), -3), (dict(mode=4), -3), (dict(mode=5), -1), (dict(mode=-2), -1), (dict(a=2), -1), (dict(mode=3, sid_mode=3), -1),
                     (dict(a=1, sid_mode=-1), -1)):
        with pytest.raises(api.MkError, match="error %d" % code):
            api.search(e2e.db, q, _params(api, **kw))
    # profile queries (the inverted search) refuse the backtrace by name
    for kw in (dict(mode=3), dict(a=1)):
        p = _params(api, profile_search=1, **kw)
        with pytest.raises(api.MkError, match="error -3") as e:
            api.TargetDB(e2e.targets[:20], p)
        assert "profile" in str(e.value)
        with pytest.raises(api.MkError, match="error -3"):
            api.search(e2e.db, q, p)


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
    """`align -a 1 --alignment-mode 3` on the real process's own prefilter result (also with the host assembly forced), `search`, and
    `predictexons --alignment-mode 3 -a 1` with and without --min-seq-id 0.3 --seq-id-mode 1, against the DBs the real binary wrote"""
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
    argv = ["-a", "1", "--alignment-mode", "3", "-e", "100", "--min-aln-len", "11", "--seq-id-mode", "0", "--threads", "4", "--ref-l2-bytes", str(L2)]
    subprocess.check_call([build.BIN, "align", t + "aa_6f", t + "targets", t + "pref_0", t + "res"] + argv, stderr=subprocess.DEVNULL)
    assert blocks(_read_result_db(t + "res")) == _text("e2e_process_aln_m3a.txt.gz")
    subprocess.check_call([build.BIN, "align", t + "aa_6f", t + "targets", t + "pref_0", t + "res_host"] + argv, stderr=subprocess.DEVNULL,
                          env=dict(os.environ, MK_DEBUG="1", MK_ALIGN_HOST_ASSEMBLE="1"))
    assert open(t + "res_host", "rb").read() == open(t + "res", "rb").read()
    subprocess.check_call([build.BIN, "search", t + "aa_6f", t + "targets", t + "res_search", t + "tmp", "-s", "5.7"] + argv, stderr=subprocess.DEVNULL)
    assert blocks(_read_result_db(t + "res_search")) == _text("e2e_process_aln_m3a.txt.gz")
    pe = ["--threads", "4", "--ref-l2-bytes", str(L2), "-s", "5.7", "--alignment-mode", "3", "-a", "1"]
    subprocess.check_call([build.BIN, "predictexons", t + "contigs", t + "targets", t + "calls", t + "tmp"] + pe, stderr=subprocess.DEVNULL)
    assert blocks(_read_result_db(t + "calls")) == _text("e2e_process_calls_m3a.txt.gz")
    subprocess.check_call([build.BIN, "predictexons", t + "contigs", t + "targets", t + "calls2", t + "tmp"] + pe + ["--min-seq-id", "0.3", "--seq-id-mode", "1"],
                          stderr=subprocess.DEVNULL)
    assert blocks(_read_result_db(t + "calls2")) == _text("e2e_process_calls_m3a_id03.txt.gz")
    assert _text("e2e_process_calls_m3a_id03.txt.gz") != _text("e2e_process_calls_m3a.txt.gz")
    # refused by name: the modes that are not built, the backtrace column in swapresults
    for bad in (["--alignment-mode", "0"], ["--alignment-mode", "1"], ["--alignment-mode", "4"], ["--seq-id-mode", "3"]):
        r = subprocess.run([build.BIN, "align", t + "aa_6f", t + "targets", t + "pref_0", t + "res_bad"] + [x for x in argv if x not in ("--alignment-mode", "3", "--seq-id-mode", "0")] + bad
                           + ([] if bad[0] == "--alignment-mode" else ["--alignment-mode", "3"]), stderr=subprocess.PIPE)
        assert r.returncode != 0 and bad[0].encode() in r.stderr, (bad, r.stderr[-300:])
    r = subprocess.run([build.BIN, "swapresults", t + "aa_6f", t + "targets", t + "res", t + "swapped"], stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"backtrace" in r.stderr, r.stderr[-300:]
