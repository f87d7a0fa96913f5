"""--alignment-mode 3 / -a without a GPU: the host restatement of the banded backtrace (mk_backtrace_host: SmithWaterman::banded_sw +
computerBacktrace) against the records the REAL `metaeuk` binary wrote (tests/golden/make_backtrace_golden.sh), the parameters' checks and the
11-column formatter.

The inputs of every call come from the parity oracle, not from the library: the alignment matrix, the query's int8 composition bias
(mko_sw_query_init), the raw score and the coordinates of the pair (mko_align_pair).  The expected side is the fixture's text."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import oracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


def _text(name):
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        return f.read()


def _lines(name):
    return _text(name).split("\n")[:-1]


def _blocks(text):
    """'>key' blocks -> {key: [lines]}"""
    out, cur = {}, None
    for ln in text.splitlines():
        if ln.startswith(">"):
            cur = out.setdefault(int(ln[1:]), [])
        else:
            cur.append(ln)
    return out


def compress(ops):
    """Matcher::compressAlignment"""
    return "".join("%d%s" % (len(m.group(0)), m.group(0)[0]) for m in re.finditer(r"M+|I+|D+", ops))


def printed_identity(x):
    """Util::fastSeqIdToBuffer on a float32 in [0, 1]"""
    return "1.00" if x == F(1.0) else "0.%03d" % int(F(x) * F(1000))


class AlnResult(C.Structure):
    _fields_ = [("db_key", C.c_uint32), ("bit_score", C.c_int), ("seq_id", C.c_float), ("evalue", C.c_double), ("q_start", C.c_int), ("q_end", C.c_int),
                ("q_len", C.c_int), ("db_start", C.c_int), ("db_end", C.c_int), ("db_len", C.c_int), ("aln_len", C.c_int), ("qcov", C.c_float),
                ("dbcov", C.c_float), ("raw_score", C.c_int)]


class AlignCtx(C.Structure):
    _fields_ = [("mat", C.c_void_p), ("evaluer", C.c_void_p), ("gap_open", C.c_int), ("gap_extend", C.c_int), ("eval_thr", C.c_double),
                ("aln_len_thr", C.c_int), ("lanes_byte", C.c_int), ("lanes_word", C.c_int), ("bias_scale", C.c_float)]


class Traced:
    """every record of a fixture through mko_align_pair (coordinates, raw score) and mk_backtrace_host"""

    def __init__(self, api, queries, targets, aln_text):
        L = oracle.lib()
        self.m = oracle.submat(0, 2.0, 0.0)
        self.mat = np.array([[self.m.sub[i][j] for j in range(21)] for i in range(21)], dtype=np.int8)
        ev = (C.c_double * 32)()
        L.mko_evaluer_init(ev, C.c_uint64(sum(len(t) for t in targets)))
        ctx = AlignCtx(C.cast(C.byref(self.m), C.c_void_p), C.cast(ev, C.c_void_p), 11, 1, 1e300, 0, 32, 16, 1.0)
        tcodes = {}
        self.rows = []                # (query key, line, ops or None, identities, attempts, q_len, t_len)
        for qk, lines in sorted(_blocks(aln_text).items()):
            qc = oracle.encode(queries[qk])
            cb = np.zeros(max(1, len(qc)), dtype=np.int8)
            bias = C.c_int()
            L.mko_sw_query_init(C.byref(self.m), qc.ctypes.data_as(C.c_void_p), C.c_int(len(qc)), C.c_float(1.0), cb.ctypes.data_as(C.c_void_p), C.byref(bias))
            for ln in lines:
                c = ln.split("\t")
                tk = int(c[0])
                if tk not in tcodes:
                    tcodes[tk] = oracle.encode(targets[tk])
                tc = tcodes[tk]
                r = AlnResult()
                L.mko_align_pair(C.byref(ctx), qc.ctypes.data_as(C.c_void_p), cb.ctypes.data_as(C.c_void_p), bias, C.c_int(len(qc)),
                                 tc.ctypes.data_as(C.c_void_p), C.c_int(len(tc)), C.c_uint32(tk), C.byref(r))
                assert [r.q_start, r.q_end, r.q_len, r.db_start, r.db_end, r.db_len] == [int(x) for x in c[4:10]], ln
                ops, ids, att = api.backtrace_host(self.mat, qc[r.q_start:r.q_end + 1], cb[r.q_start:r.q_end + 1], tc[r.db_start:r.db_end + 1], r.raw_score)
                self.rows.append((qk, ln, None if ops is None else ops.decode(), ids, att, len(qc), len(tc)))


@pytest.fixture(scope="module")
def api():
    from metaeuk_amd import api
    return api


@pytest.fixture(scope="module")
def corner(api):
    return Traced(api, _lines("bt_corner_queries.txt.gz"), _lines("bt_corner_targets.txt.gz"), _text("bt_corner_aln.txt.gz"))


@pytest.fixture(scope="module")
def e2e(api):
    frags = [l.rsplit("\t", 1)[1] for l in _lines("e2e_process_orfs.txt.gz")]
    return Traced(api, frags, _lines("e2e_targets.txt.gz"), _text("e2e_process_aln_m3a.txt.gz"))


def _check_against_lines(tr):
    left = [ln for (_, ln, ops, _, _, _, _) in tr.rows if ops is None]
    assert not left, ("the trace left the band", len(left), left[:3])
    bad = []
    for qk, ln, ops, ids, att, ql, tl in tr.rows:
        c = ln.split("\t")
        if compress(ops) != c[10] or printed_identity(F(ids) / F(len(ops))) != c[2]:
            bad.append((qk, ln, compress(ops), ids, len(ops)))
    assert not bad, (len(bad), bad[:3])


def test_host_backtrace_equals_the_corner_fixture(corner):
    assert len(corner.rows) == 2248
    _check_against_lines(corner)


def test_host_backtrace_equals_the_e2e_fixture(e2e):
    assert len(e2e.rows) == 4169
    assert sum(1 for r in e2e.rows if "I" in r[2] or "D" in r[2]) == 671
    _check_against_lines(e2e)


def test_seq_id_mode_1_and_min_seq_id_derive_the_filtered_fixture(e2e):
    """--min-seq-id 0.3 --seq-id-mode 1: identities / min(query length, target length) in float32, kept when >= the float32 threshold; the
    kept records print that identity (Util::computeSeqId, Alignment::checkCriteria)"""
    want = _blocks(_text("e2e_process_aln_m3a_id03.txt.gz"))
    got = {}
    for qk, ln, ops, ids, att, ql, tl in e2e.rows:
        sid = F(ids) / F(min(ql, tl))
        if float(sid) >= float(F(0.3)):
            c = ln.split("\t")
            c[2] = printed_identity(sid)
            got.setdefault(qk, []).append("\t".join(c))
    assert sum(len(v) for v in want.values()) == sum(len(v) for v in got.values())
    assert 100 <= sum(len(v) for v in got.values()) <= 4169 - 100
    assert got == {k: v for k, v in want.items() if v}


def test_attempt_counts_of_the_corner_classes(corner):
    """class b (3-residue indels on a square rectangle) walks the bands 1, 2, 4; class c (40-residue indels) 1, 2, 4, ..., 64"""
    cls = _text("bt_corner_classes.txt.gz").split()
    own = {}
    for qk, ln, ops, ids, att, ql, tl in corner.rows:
        if int(ln.split("\t")[0]) == qk:
            own.setdefault(cls[qk], []).append((att, ops))
    assert len(own["b"]) == 60 and len(own["c"]) == 60
    assert all(att >= 3 for att, _ in own["b"]), sorted(att for att, _ in own["b"])[:5]
    assert all(att >= 7 for att, _ in own["c"]), sorted(att for att, _ in own["c"])[:5]
    assert all("I" in ops and "D" in ops for att, ops in own["b"] + own["c"])
    assert all(att == 1 and set(ops) == {"M"} for att, ops in own["a"])
    assert any("I" in ops or "D" in ops for _, ops in own["d"]) and any("I" in ops or "D" in ops for _, ops in own["e"])


def test_one_cell_and_stalled_band(api):
    m = oracle.submat(0, 2.0, 0.0)
    mat = np.array([[m.sub[i][j] for j in range(21)] for i in range(21)], dtype=np.int8)
    a = oracle.encode("W")
    ops, ids, att = api.backtrace_host(mat, a, np.zeros(1, dtype=np.int8), a, int(mat[a[0], a[0]]))
    assert (ops, ids, att) == (b"M", 1, 1)
    # a score no band can reach: the reference doubles until its size overflows and exits
    with pytest.raises(api.MkError) as e:
        api.backtrace_host(mat, oracle.encode("WWWW"), np.zeros(4, dtype=np.int8), oracle.encode("WWWWWW"), 1000)
    assert "error -4" in str(e.value) and "not consensus" in str(e.value)


def test_parameters(api):
    p = api.default_params()
    assert (p.alignment_mode, p.add_backtrace, p.seq_id_mode, p.pad_, p.pad2_) == (0, 0, 0, 0, 0)
    assert C.sizeof(api.Params) == api.lib().mk_debug_params_size() and C.sizeof(api.Params) % 8 == 0
    names = [f[0] for f in api.Params._fields_]
    assert names.index("pad_") == names.index("alignment_mode") - 1 and names[-4:] == ["alignment_mode", "add_backtrace", "seq_id_mode", "pad2_"]

    def code(**kw):
        p = api.default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return api.lib().mk_result_filter(C.byref(p), C.c_int(50), C.c_int(60), None)
    assert [code(alignment_mode=m) for m in (0, 2, 3)] == [1, 1, 1] and code(add_backtrace=1) == 1
    assert [code(alignment_mode=3, seq_id_mode=m) for m in (0, 1, 2)] == [1, 1, 1]
    assert code(alignment_mode=1) == -3 and code(alignment_mode=4) == -3 and b"--alignment-mode 4" in api.lib().mk_last_error()
    assert code(alignment_mode=5) == -1 and code(alignment_mode=-1) == -1
    assert code(add_backtrace=2) == -1 and code(add_backtrace=-1) == -1
    assert code(alignment_mode=3, seq_id_mode=3) == -1 and code(add_backtrace=1, seq_id_mode=-1) == -1
    assert code(alignment_mode=2, seq_id_mode=7) == 1          # read in mode 3 only


def test_format_alignment_bt(api, corner, e2e):
    """the 11-column line from the 10 printed columns of a fixture record and the operations of the host restatement"""
    seen = set()
    rows = corner.rows[::7] + e2e.rows[::23] + [r for r in corner.rows + e2e.rows if r[1].split("\t")[10].endswith("D1M") or set(r[2]) == {"M"}][:40]
    for qk, ln, ops, ids, att, ql, tl in rows:
        c = ln.split("\t")
        a = api.Alignment(db_key=int(c[0]), bit_score=int(c[1]), seq_id=F(ids) / F(len(ops)), evalue=float(c[3]), q_start=int(c[4]), q_end=int(c[5]),
                          q_len=int(c[6]), db_start=int(c[7]), db_end=int(c[8]), db_len=int(c[9]))
        if "%.3E" % a.evalue != c[3]:
            continue                                  # (the printed e-value does not round-trip: not what this test is about)
        assert api.format_alignment_bt(a, ops.encode()) == (ln + "\n").encode()
        seen.add("gap" if ("I" in ops or "D" in ops) else "plain")
    assert seen == {"gap", "plain"}
    a = api.Alignment(db_key=3, bit_score=20, seq_id=1.0, evalue=1e-3, q_start=0, q_end=0, q_len=9, db_start=5, db_end=5, db_len=40)
    assert api.format_alignment_bt(a, b"M") == b"3\t20\t1.00\t1.000E-03\t0\t0\t9\t5\t5\t40\t1M\n"
    assert api.format_alignment_bt(a, b"MMMIIDM").endswith(b"\t3M2I1D1M\n")
