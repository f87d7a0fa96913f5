"""CPU test: the result filters -c / --cov-mode / --min-seq-id as mk_result_filter decides them (include/metaeuk_amd.h), against a numpy float32
restatement of Util::canBeCovered / Util::hasCoverage (M/src/commons/Util.cpp:477-511) and Alignment::checkCriteria's identity test."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import oracle
from metaeuk_amd import api

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
THRESHOLDS = [0.0, 0.5, 0.8, 0.3]                    # 0.3 is not representable: the float32 parameter is what both sides compare with
LENGTHS = [(50, 100), (100, 50), (80, 100), (100, 80), (30, 100), (100, 30), (77, 77), (1, 1), (1, 100), (100, 1), (299, 1000), (301, 1000)]


def can_be_covered(thr, mode, q_len, t_len):
    thr, q, t = F(thr), F(q_len), F(t_len)
    if mode == 0:
        return bool(q / t >= thr and t / q >= thr)
    if mode == 1:
        return bool(q / t >= thr)
    if mode == 2:
        return bool(t / q >= thr)
    if mode == 3:
        return bool(t / q >= thr and t / q <= F(1.0))
    if mode == 4:
        return bool(q / t >= thr and q / t <= F(1.0))
    return bool(min(q, t) / max(q, t) >= thr)


def has_coverage(thr, mode, qcov, dbcov):
    thr = F(thr)
    if mode == 0:
        return bool(F(qcov) >= thr and F(dbcov) >= thr)
    if mode == 1:
        return bool(F(dbcov) >= thr)
    if mode == 2:
        return bool(F(qcov) >= thr)
    return True


def keep(thr, mode, id_thr, q_len, t_len, qcov=None, dbcov=None, seq_id=None):
    if not can_be_covered(thr, mode, q_len, t_len):
        return False
    if qcov is None:
        return True
    return has_coverage(thr, mode, qcov, dbcov) and float(F(seq_id)) >= float(F(id_thr))


def _params(thr=0.0, mode=0, id_thr=0.0):
    p = api.default_params()
    p.cov_thr, p.cov_mode, p.seq_id_thr = thr, mode, id_thr
    return p


def _below(x):
    return float(np.nextafter(F(x), F(-1.0)))


def test_default_params_leave_the_filters_off():
    p = api.Params()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    api.lib().mk_default_params(C.byref(p))
    assert (p.cov_thr, p.cov_mode, p.seq_id_thr, p.pad_) == (0.0, 0, 0.0, 0)
    assert p.kmer_size == 0 and p.profile_search == 0 and p.max_seqs == 300          # the fields in front of them did not move


def test_binding_mirrors_the_struct():
    assert C.sizeof(api.Params) == api.lib().mk_debug_params_size()
    assert api.Params.cov_thr.offset == api.Params.kmer_size.offset + 4               # appended behind the last field of the parent layout


@pytest.mark.parametrize("bad", [dict(mode=6), dict(mode=-1), dict(thr=1.5), dict(thr=-0.1), dict(id_thr=1.01), dict(thr=float("nan"))])
def test_values_out_of_range_are_an_argument_error(bad):
    p = _params(**bad)
    assert api.lib().mk_result_filter(C.byref(p), C.c_int(50), C.c_int(100), None) == -1           # MK_ERR_ARG
    assert b"--cov-mode" in api.lib().mk_last_error()
    with pytest.raises(api.MkError):
        api.result_filter(p, 50, 100)


@pytest.mark.parametrize("mode", range(6))
def test_length_test_matrix(mode):
    cells = 0
    for thr in THRESHOLDS:
        p = _params(thr, mode)
        for q_len, t_len in LENGTHS:
            assert api.result_filter(p, q_len, t_len) == can_be_covered(thr, mode, q_len, t_len), (thr, mode, q_len, t_len)
            cells += 1
    assert cells == len(THRESHOLDS) * len(LENGTHS)
    # the boundary by hand: a ratio of exactly 0.5 passes -c 0.5; only the `<= 1.0` clause of modes 3 / 4 rejects the pair the wrong way round
    assert api.result_filter(_params(0.5, mode), 50, 100) == (mode != 3)      # q / t = 0.5, t / q = 2
    assert api.result_filter(_params(0.5, mode), 100, 50) == (mode != 4)
    assert not api.result_filter(_params(0.5, mode), 49, 100) or mode in (2, 3)      # 0.49 fails wherever q / t is looked at (mode 3 fails on t / q > 1)
    assert api.result_filter(_params(0.5, 2), 49, 100) and not api.result_filter(_params(0.5, 3), 49, 100)


@pytest.mark.parametrize("mode", range(6))
def test_alignment_matrix(mode):
    """coverage and identity exactly on the threshold and one ulp below it, for lengths that pass the length test"""
    checked = dropped = 0
    for thr in THRESHOLDS:
        for id_thr in THRESHOLDS:
            p = _params(thr, mode, id_thr)
            on, under = float(F(thr)), _below(thr) if thr > 0 else 0.0
            id_on, id_under = float(F(id_thr)), _below(id_thr) if id_thr > 0 else 0.0
            for q_len, t_len in LENGTHS:
                for qcov in (on, under, 1.0):
                    for dbcov in (on, under, 1.0):
                        for sid in (id_on, id_under, 1.0):
                            a = api.Alignment(qcov=qcov, dbcov=dbcov, seq_id=sid, q_len=q_len, db_len=t_len)
                            want = keep(thr, mode, id_thr, q_len, t_len, qcov, dbcov, sid)
                            assert api.result_filter(p, q_len, t_len, a) == want, (thr, mode, id_thr, q_len, t_len, qcov, dbcov, sid)
                            checked += 1
                            dropped += not want
    assert checked == len(THRESHOLDS) ** 2 * len(LENGTHS) * 27 and 0 < dropped < checked


def test_one_ulp_decides():
    a = api.Alignment(qcov=0.5, dbcov=0.5, seq_id=0.5)
    assert api.result_filter(_params(0.5, 0, 0.5), 80, 100, a)
    for field in ("qcov", "dbcov", "seq_id"):
        b = api.Alignment(qcov=0.5, dbcov=0.5, seq_id=0.5)
        setattr(b, field, _below(0.5))
        assert not api.result_filter(_params(0.5, 0, 0.5), 80, 100, b), field
    # the length modes never look at the coverage of the alignment (Util::hasCoverage)
    b = api.Alignment(qcov=0.01, dbcov=0.01, seq_id=1.0)
    for mode in (3, 4, 5):
        assert api.result_filter(_params(0.5, mode), 100, 100, b)
    # ... and keep their `<= 1.0` clause at -c 0
    assert not api.result_filter(_params(0.0, 3), 50, 100) and api.result_filter(_params(0.0, 3), 100, 50)
    assert not api.result_filter(_params(0.0, 4), 100, 50) and api.result_filter(_params(0.0, 4), 50, 100)


def test_counts_on_the_small_fixture():
    """the predicates of this file on the printed columns of tests/golden/small_aln.txt.gz (437 unfiltered alignments): what the GPU tests
    expect of every coverage mode at -c 0.5, and of --min-seq-id 0.5"""
    with gzip.open(os.path.join(GOLD, "small_targets.txt.gz"), "rt") as f:
        targets = f.read().split("\n")[:-1]
    with gzip.open(os.path.join(GOLD, "small_queries.txt.gz"), "rt") as f:
        queries = f.read().split("\n")[:-1]
    blocks = oracle.read_blocks(os.path.join(GOLD, "small_aln.txt.gz"))
    assert len(blocks) == len(queries)
    recs = [ln.split("\t") for b in blocks for ln in b.splitlines()]
    assert len(recs) == 437
    kept = [0] * 6
    for c in recs:
        qs, qe, ql, ts, te, tl = (int(x) for x in c[4:10])
        assert tl == len(targets[int(c[0])])
        qcov, dbcov = F(qe - qs + 1) / F(ql), F(te - ts + 1) / F(tl)
        a = api.Alignment(qcov=float(qcov), dbcov=float(dbcov), seq_id=float(c[2]), q_len=ql, db_len=tl)
        for mode in range(6):
            k = keep(0.5, mode, 0.0, ql, tl, qcov, dbcov, 1.0)
            assert api.result_filter(_params(0.5, mode), ql, tl, a) == k
            kept[mode] += k
    assert kept == [68, 68, 306, 15, 115, 130]
