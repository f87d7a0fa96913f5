"""The result filters -c / --cov-mode / --min-seq-id on the GPU search path (mk_params.cov_thr / cov_mode / seq_id_thr).

The expected side never comes from the library: it is the oracle's (or the real `metaeuk` binary's) UNFILTERED result with the failing records
removed by predicates computed here from the printed integer columns -- coverage = (end - start + 1) / len in float32 (compute_cov,
oracle/mko_align.c:207), the length test of Util::canBeCovered on the two lengths, the identity from the printed third column.  With
--alignment-mode 2 and the accept / reject counters at their defaults the reference's filtered result is exactly that (Alignment.cpp:343-405,
548-567): the early exits change cost, never content."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import oracle
from test_result_filters_host import can_be_covered, has_coverage

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32
L2 = 2097152                                       # tests/golden/PROVENANCE.txt
PREF_CUT_MODES = (0, 2, 5)                         # Prefiltering.cpp:856-863


def _lines(name):
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        return f.read().split("\n")[:-1]


def _text(name):
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        return f.read()


# ---- the derivation: unfiltered text -> filtered text -------------------------------------------------------------------------------
def cut_pref_block(block, q_len, t_len_of, thr, mode):
    """a query's prefilter lines ('key score diagonal') without the targets whose length cannot reach the threshold"""
    if not (thr > 0 and mode in PREF_CUT_MODES):
        return block
    return "".join(ln for ln in block.splitlines(True) if can_be_covered(thr, mode, q_len, t_len_of(int(ln.split("\t")[0]))))


def aln_line_passes(ln, thr, mode, id_thr):
    c = ln.rstrip("\n").split("\t")
    qs, qe, ql, ts, te, tl = (int(x) for x in c[4:10])
    if not can_be_covered(thr, mode, ql, tl):
        return False
    qcov, dbcov = F(qe - qs + 1) / F(ql), F(te - ts + 1) / F(tl)
    # the identity is printed as floor(1000 x) / 1000: for a threshold with at most three decimals that float32 holds exactly (0.5) the printed
    # value decides
    return has_coverage(thr, mode, qcov, dbcov) and float(c[2]) >= id_thr


def cut_aln_block(block, thr, mode, id_thr):
    return "".join(ln for ln in block.splitlines(True) if aln_line_passes(ln, thr, mode, id_thr))


def _n(blocks):
    return sum(b.count("\n") for b in blocks)


# ---- fixture: the `small` golden inputs, the oracle's unfiltered run, one database ---------------------------------------------------
class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(gpu_api, tmp_path_factory):
    c = Ctx()
    c.api = gpu_api
    c.targets, c.queries = _lines("small_targets.txt.gz"), _lines("small_queries.txt.gz")
    c.pref, c.aln = oracle.run_pipeline(c.targets, c.queries, str(tmp_path_factory.mktemp("oracle_unfiltered")), extra=["--l2", str(L2)])
    assert len(c.pref) == len(c.queries) == len(c.aln) and _n(c.aln) == 437
    base = gpu_api.default_params()
    base.host_l2_bytes = L2
    c.db = gpu_api.TargetDB(c.targets, base)
    return c


def _params(c, thr=0.0, mode=0, id_thr=0.0):
    p = c.api.default_params()
    p.host_l2_bytes = L2
    p.cov_thr, p.cov_mode, p.seq_id_thr = thr, mode, id_thr
    return p


def _expected(c, thr, mode, id_thr, lo=0, hi=None):
    hi = len(c.queries) if hi is None else hi
    pref = [cut_pref_block(c.pref[i], len(c.queries[i]), lambda t: len(c.targets[t]), thr, mode) for i in range(lo, hi)]
    aln = [cut_aln_block(c.aln[i], thr, mode, id_thr) for i in range(lo, hi)]
    return pref, aln


def _formatted(api, result, n):
    (hits, hoff), (alns, aoff) = result
    return ([api.format_hits(hits, int(hoff[i]), int(hoff[i + 1])) for i in range(n)],
            [api.format_alignments(alns, int(aoff[i]), int(aoff[i + 1])) for i in range(n)])


def _check(got, want):
    for name, g, w in (("pref", got[0], want[0]), ("aln", got[1], want[1])):
        bad = [i for i in range(len(w)) if g[i] != w[i]]
        assert not bad, (name, bad[:10], g[bad[0]], w[bad[0]])


def _search(c, p, queries=None):
    queries = c.queries if queries is None else queries
    q = c.api.Queries(queries, p)
    return _formatted(c.api, c.api.search(c.db, q, p), len(queries))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", range(6))
def test_every_coverage_mode(ctx, mode):
    want = _expected(ctx, 0.5, mode, 0.0)
    kept, dropped = _n(want[1]), 437 - _n(want[1])
    print("cov-mode %d: %d alignments kept, %d dropped; prefilter hits %d of %d" % (mode, kept, dropped, _n(want[0]), _n(ctx.pref)))
    assert kept >= 10 and dropped >= 100
    assert kept == [68, 68, 306, 15, 115, 130][mode]
    # the prefilter's cut exists for modes 0, 2 and 5 only (every protein of the fixture is longer than half a fragment: mode 2 finds nothing to cut)
    assert want[0] == ctx.pref if mode not in PREF_CUT_MODES else _n(want[0]) <= _n(ctx.pref)
    assert mode != 0 or 10 <= _n(want[0]) <= _n(ctx.pref) - 100
    _check(_search(ctx, _params(ctx, 0.5, mode)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("thr,mode", [(0.0, 0), (0.5, 0)])
def test_sequence_identity(ctx, thr, mode):
    want = _expected(ctx, thr, mode, 0.5)
    print("--min-seq-id 0.5 -c %g: %d of 437 alignments kept" % (thr, _n(want[1])))
    assert 10 <= _n(want[1]) <= 437 - 100
    if thr == 0.0:
        assert 250 <= _n(want[1]) <= 300              # "about 276"
    _check(_search(ctx, _params(ctx, thr, mode, 0.5)), want)


@pytest.mark.gpu
@pytest.mark.parametrize("front_end", ["fused", "wide", "global", "fused-tiny"])
def test_every_prefilter_front_end(ctx, monkeypatch, front_end):
    monkeypatch.setenv("MK_PREFILTER_PATH", front_end.split("-")[0])
    monkeypatch.setenv("MK_PREFILTER_TIERS", "tiny" if front_end.endswith("-tiny") else "default")
    _check(_search(ctx, _params(ctx, 0.5, 0)), _expected(ctx, 0.5, 0, 0.0))


@pytest.mark.gpu
def test_prefilter_then_align_and_queued_batches(ctx):
    api = ctx.api
    p = _params(ctx, 0.5, 0, 0.5)
    want = _expected(ctx, 0.5, 0, 0.5)
    n = len(ctx.queries)
    q = api.Queries(ctx.queries, p)
    pref = api.prefilter(ctx.db, q, p)
    _check(_formatted(api, (pref, api.align(ctx.db, q, p)), n), want)
    # the prefilter result of the caller is the cut list, and align does not touch it
    hits, hoff = api.prefilter_result(q)
    assert int(hoff[-1]) == _n(want[0])
    # two batches queued behind each other
    half = n // 2
    qa, qb = api.Queries(ctx.queries[:half], p), api.Queries(ctx.queries[half:], p)
    api.search_begin(ctx.db, qa, p)
    api.search_begin(ctx.db, qb, p)
    got_b = _formatted(api, api.search_wait(qb), n - half)
    got_a = _formatted(api, api.search_wait(qa), half)
    _check(got_a, _expected(ctx, 0.5, 0, 0.5, 0, half))
    _check(got_b, _expected(ctx, 0.5, 0, 0.5, half, n))


def _sw_cells(stats, prefix):
    return sum(v["cells"] for k, v in stats.items() if k.startswith(prefix))


def _align_launches(stats):
    return {k: v["launches"] for k, v in stats.items() if v["launches"] > 0 and (k.startswith("sw_") or k.startswith("align_"))}


@pytest.mark.gpu
def test_work_is_skipped_not_only_hidden(ctx):
    api = ctx.api
    api.kernel_stats(reset=True)
    plain = _search(ctx, _params(ctx))
    s_plain = api.kernel_stats(reset=True)
    _check(plain, (ctx.pref, ctx.aln))
    got = _search(ctx, _params(ctx, 0.8, 1))
    s_cut = api.kernel_stats(reset=True)
    _check(got, _expected(ctx, 0.8, 1, 0.0))
    for prefix in ("sw_fwd", "sw_rev"):
        a, b = _sw_cells(s_plain, prefix), _sw_cells(s_cut, prefix)
        print("%s cells: %.0f unfiltered, %.0f with -c 0.8 --cov-mode 1" % (prefix, a, b))
        assert b < a
    assert "align_cut" in s_cut and "align_cut" not in s_plain
    # (no fragment covers 80 % of a protein: that run ends at the length cut.  The coverage gate in front of the reverse pass shows with the
    #  query coverage, which the lengths rarely decide: fewer reverse cells, not none)
    got = _search(ctx, _params(ctx, 0.5, 2))
    s_gate = api.kernel_stats(reset=True)
    _check(got, _expected(ctx, 0.5, 2, 0.0))
    print("sw_rev cells: %.0f unfiltered, %.0f with -c 0.5 --cov-mode 2" % (_sw_cells(s_plain, "sw_rev"), _sw_cells(s_gate, "sw_rev")))
    assert 0 < _sw_cells(s_gate, "sw_rev") < _sw_cells(s_plain, "sw_rev")
    assert 0 < _sw_cells(s_gate, "sw_fwd") <= _sw_cells(s_plain, "sw_fwd")
    # both thresholds 0: the alignment stage launches what it launches with the fields as default_params() leaves them
    p0 = ctx.api.default_params()
    p0.host_l2_bytes = L2
    q = api.Queries(ctx.queries, p0)
    api.search(ctx.db, q, p0)
    s_default = api.kernel_stats(reset=True)
    assert _align_launches(s_default) == _align_launches(s_plain) and len(_align_launches(s_plain)) >= 5


@pytest.mark.gpu
def test_profile_search_refuses_the_filters(ctx):
    p = _params(ctx, 0.5, 0)
    p.profile_search = 1
    with pytest.raises(ctx.api.MkError, match="error -3"):                # MK_ERR_UNSUPPORTED
        ctx.api.TargetDB(ctx.targets[:20], p)
    q = ctx.api.Queries(ctx.queries[:10], _params(ctx))
    with pytest.raises(ctx.api.MkError, match="error -3"):
        ctx.api.search(ctx.db, q, p)
    bad = _params(ctx, 0.5, 6)
    with pytest.raises(ctx.api.MkError, match="error -1"):                # MK_ERR_ARG
        ctx.api.search(ctx.db, q, bad)


# ---- command line ----------------------------------------------------------------------------------------------------------------------
def _write_seq_db(base, seqs, keys=None, dbtype=0):
    keys = keys if keys is not None else list(range(len(seqs)))
    off = 0
    with open(base, "wb") as d, open(base + ".index", "w") as i:
        for k, s in zip(keys, seqs):
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


PREFILTER_ARGV = ["--sub-mat", "aa:blosum62.out,nucl:nucleotide.out", "--seed-sub-mat", "aa:VTML80.out,nucl:nucleotide.out", "-k", "0",
                  "--k-score", "seq:2147483647,prof:2147483647", "--alph-size", "aa:21,nucl:5", "--max-seq-len", "65535", "--max-seqs", "300",
                  "--split", "0", "--split-mode", "2", "--comp-bias-corr", "1", "--diag-score", "1", "--exact-kmer-matching", "0",
                  "--mask", "1", "--mask-prob", "0.9", "--min-ungapped-score", "15", "--spaced-kmer-mode", "1", "-s", "5.7", "--threads", "4",
                  "--ref-l2-bytes", str(L2)]
ALIGN_ARGV = ["--alignment-mode", "2", "-e", "100", "--min-aln-len", "11", "--max-rejected", "2147483647",
              "--max-accept", "2147483647", "--alt-ali", "0", "--realign", "0", "--gap-open", "aa:11,nucl:5", "--gap-extend", "aa:1,nucl:2",
              "--comp-bias-corr", "1", "-a", "0", "--threads", "4"]


@pytest.mark.gpu
def test_cli_prefilter_align_with_filters(ctx, tmp_path):
    """`prefilter` / `align` over MMseqs2-format DBs with the predictexons argv and -c 0.5 --cov-mode 2 --min-seq-id 0.5"""
    from metaeuk_amd import build
    queries = ctx.queries[:600]
    qkeys = [3 * i + 1 for i in range(len(queries))]
    _write_seq_db(str(tmp_path / "q"), queries, qkeys)
    _write_seq_db(str(tmp_path / "t"), ctx.targets)
    subprocess.check_call([build.BIN, "prefilter", str(tmp_path / "q"), str(tmp_path / "t"), str(tmp_path / "pref_0")] + PREFILTER_ARGV + ["-c", "0.5", "--cov-mode", "2"])
    subprocess.check_call([build.BIN, "align", str(tmp_path / "q"), str(tmp_path / "t"), str(tmp_path / "pref_0"), str(tmp_path / "res")] + ALIGN_ARGV +
                          ["-c", "0.5", "--cov-mode", "2", "--min-seq-id", "0.5"])
    pref, res = _read_result_db(str(tmp_path / "pref_0")), _read_result_db(str(tmp_path / "res"))
    want = _expected(ctx, 0.5, 2, 0.5, 0, 600)
    assert sorted(pref) == qkeys and sorted(res) == qkeys
    assert 10 <= _n(want[1]) < _n(ctx.aln[:600]) and 10 <= _n(want[0])
    _check(([pref[k] for k in qkeys], [res[k] for k in qkeys]), want)
    # the host assembly (what a range with a score beyond the e-value table falls back to) reads the stage's cut list and decides with mk_result_filter
    subprocess.check_call([build.BIN, "align", str(tmp_path / "q"), str(tmp_path / "t"), str(tmp_path / "pref_0"), str(tmp_path / "res_host")] + ALIGN_ARGV +
                          ["-c", "0.5", "--cov-mode", "0", "--min-seq-id", "0.5"], env=dict(os.environ, MK_DEBUG="1", MK_ALIGN_HOST_ASSEMBLE="1"))
    res_host = _read_result_db(str(tmp_path / "res_host"))
    assert [res_host[k] for k in qkeys] == _expected(ctx, 0.5, 0, 0.5, 0, 600)[1]
    # `search` (the two modules as one pass) writes the same alignment DB
    subprocess.check_call([build.BIN, "search", str(tmp_path / "q"), str(tmp_path / "t"), str(tmp_path / "res2"), str(tmp_path / "tmp")] + ALIGN_ARGV +
                          ["-s", "5.7", "--ref-l2-bytes", str(L2), "-c", "0.5", "--cov-mode", "2", "--min-seq-id", "0.5"])
    res2 = _read_result_db(str(tmp_path / "res2"))
    assert [res2[k] for k in qkeys] == want[1]
    # a coverage mode that does not exist is a hard error and leaves no "done" marker behind
    bad = subprocess.run([build.BIN, "prefilter", str(tmp_path / "q"), str(tmp_path / "t"), str(tmp_path / "x"), "-c", "0.5", "--cov-mode", "7"], capture_output=True)
    assert bad.returncode != 0 and not (tmp_path / "x.dbtype").exists() and b"--cov-mode" in bad.stderr


# ---- the real process: `metaeuk predictexons ... -c 0.5 --cov-mode 0 --min-seq-id 0.3` (tests/golden/make_filter_golden.sh) ------------
def _blocks_of(text):
    out, cur = {}, None
    for ln in text.splitlines(True):
        if ln.startswith(">"):
            cur = int(ln[1:])
            out[cur] = ""
        else:
            out[cur] += ln
    return out


EDGE = ("0.299", "0.300")                          # printed identities the float32 threshold 0.3 may cut either way


def test_filtered_process_fixtures_equal_the_unfiltered_ones_cut_here():
    """ties the derivation every other test uses to the real binary: its filtered pref_0 / search_res are its unfiltered ones with the failing
    lines removed by the predicates of this file"""
    targets = _lines("e2e_targets.txt.gz")
    frag_len = [len(ln.split("\t")[-1]) for ln in _lines("e2e_process_orfs.txt.gz")]          # "header<TAB>protein" per fragment, by key
    pref, pref_cut = _blocks_of(_text("e2e_process_pref.txt.gz")), _blocks_of(_text("e2e_process_pref_c05.txt.gz"))
    assert sorted(pref) == sorted(pref_cut) and len(pref) == len(frag_len)
    for k in pref:
        assert cut_pref_block(pref[k], frag_len[k], lambda t: len(targets[t]), 0.5, 0) == pref_cut[k], k
    n_pref, n_cut = _n(pref.values()), _n(pref_cut.values())
    assert 0 < n_cut < n_pref
    aln, aln_cut = _blocks_of(_text("e2e_process_aln.txt.gz")), _blocks_of(_text("e2e_process_aln_c05_id03.txt.gz"))
    assert sorted(aln) == sorted(aln_cut) and _n(aln.values()) == 4169
    both = sum(1 for b in aln.values() for ln in b.splitlines() if aln_line_passes(ln, 0.5, 0, 0.0))
    assert both == 865                                # both coverages >= 0.5
    edge = 0
    off_edge = lambda b: [ln for ln in b.splitlines() if ln.split("\t")[2] not in EDGE]
    for k in aln:
        edge += len(aln[k].splitlines()) - len(off_edge(aln[k]))
        want = [ln for ln in off_edge(aln[k]) if aln_line_passes(ln, 0.5, 0, 0.3)]
        assert want == off_edge(aln_cut[k]), k
    assert edge <= 0.01 * 4169, edge
    assert 10 <= _n(aln_cut.values()) <= both


@pytest.mark.gpu
def test_cli_equals_the_real_process_with_filters(gpu_api, tmp_path):
    """the commands with the real binary's flags over DBs written from e2e_contigs / e2e_targets: pref_0, search_res and the exon sets byte for byte"""
    from metaeuk_amd import build
    targets, contigs = _lines("e2e_targets.txt.gz"), _lines("e2e_contigs.txt.gz")
    _write_seq_db(str(tmp_path / "targets"), targets)
    _write_seq_db(str(tmp_path / "contigs"), contigs, dbtype=1)
    run = lambda *a: subprocess.check_call([build.BIN] + [str(x) for x in a], stderr=subprocess.DEVNULL)
    run("extractorfs", tmp_path / "contigs", tmp_path / "aa_6f", "--translate", "1", "--min-length", "15", "--max-length", "32734", "--max-gaps", "2147483647",
        "--contig-start-mode", "2", "--contig-end-mode", "2", "--orf-start-mode", "1", "--forward-frames", "1,2,3", "--reverse-frames", "1,2,3",
        "--translation-table", "1", "--use-all-table-starts", "0", "--id-offset", "0", "--create-lookup", "0", "--threads", "4", "--compressed", "0", "-v", "3")
    run("prefilter", tmp_path / "aa_6f", tmp_path / "targets", tmp_path / "pref_0", *PREFILTER_ARGV, "-c", "0.5", "--cov-mode", "0")
    blocks = lambda d: "".join(">%d\n%s" % (k, d[k]) for k in sorted(d))
    assert blocks(_read_result_db(str(tmp_path / "pref_0"))) == _text("e2e_process_pref_c05.txt.gz")
    run("align", tmp_path / "aa_6f", tmp_path / "targets", tmp_path / "pref_0", tmp_path / "search_res", *ALIGN_ARGV, "--ref-l2-bytes", L2,
        "-c", "0.5", "--cov-mode", "0", "--min-seq-id", "0.3")
    assert blocks(_read_result_db(str(tmp_path / "search_res"))) == _text("e2e_process_aln_c05_id03.txt.gz")
    run("predictexons", tmp_path / "contigs", tmp_path / "targets", tmp_path / "calls", tmp_path / "tmp", "--threads", "4", "--ref-l2-bytes", L2,
        "-s", "5.7", "-c", "0.5", "--cov-mode", "0", "--min-seq-id", "0.3")
    assert blocks(_read_result_db(str(tmp_path / "calls"))) == _text("e2e_process_calls_c05_id03.txt.gz")
