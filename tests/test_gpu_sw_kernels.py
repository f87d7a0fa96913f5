"""The alignment stage on the hand-made lists of tests/sw_cases.py, pair by pair against the oracle: the packed score pass (swp_kernel, every
tile shape), the packed known-score position / reverse pass (swq_kernel), the early exit of the int32 wavefront, the one-launch-per-class
form (sw_multi_kernel), the transposed kernels of profile queries (swt_kernel / swtp_kernel) and the planner that cuts the lists into waves
-- the code mk_sw_pairs does not run.  prefilter_result_set installs the lists, -e DBL_MAX and --min-aln-len 0 let every positive score
through, and every form of the stage must give the oracle's (score, q_start, q_end, db_start, db_end) for every pair: there is a record
if and only if the oracle's score is above 0.  tests/test_sw_cases_host.py holds the conditions under which this cannot pass by accident."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sw_cases as sc

pytestmark = pytest.mark.gpu
DBL_MAX = 1.7976931348623157e308
GROUPS = sorted(sc.SEQUENCE_GROUPS)
GROUP_LANES = [(g, lanes) for g in GROUPS for lanes in sc.lanes_of(g)]
# (MK_SW_EARLY_EXIT, MK_SW_KNOWN and the full DP launch kernels of the same names as the default and the library reports nothing else about them:
#  only the multi and the transposed forms can be confirmed through kernel_stats(); the others are trusted to the switches of mk_align.hip)
# the forms whose switch is read once per process (align_shapes() of mk_align.hip): fresh child processes
CHILD_FORMS = {"known": dict(MK_SW_KNOWN="1"),
               "int32": dict(MK_SW_KNOWN="0"),
               "multi": dict(MK_SW_KNOWN="0", MK_SW_MULTI="1"),
               "full-dp": dict(MK_SW_KNOWN="0", MK_SW_EARLY_EXIT="0")}
MULTI_MAX_ROWS = 1024                    # the one-launch-per-class form does not take batches with a query beyond the largest tile


def _params(api, cs, lanes=(32, 16)):
    p = api.default_params()
    p.evalue_thr = DBL_MAX
    p.min_aln_len = 0
    p.simd_lanes_byte, p.simd_lanes_word = lanes
    if isinstance(cs, sc.ProfileSet):
        p.profile_search = 1
        p.max_seqs = max(300, len(cs.targets))
    else:
        p.gap_open, p.gap_extend = cs.gap_open, cs.gap_extend
        if not cs.bias:
            p.comp_bias_corr = 0
    return p


def _hit_lists(api, lists):
    off = np.zeros(len(lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(l) for l in lists])
    hits = np.zeros(int(off[-1]), dtype=api.HIT_DTYPE)
    hits["seq_id"] = [t for l in lists for t in l]
    return hits, off


_DBS = {}


def _db(api, cs, lanes):
    key = (cs.name, lanes)
    if key not in _DBS:
        _DBS[key] = api.TargetDB(cs.targets, _params(api, cs, lanes))
    return _DBS[key]


def _align(api, cs, lanes, keep, lists):
    """align on `lists` (one per query of `keep`) -> ({(query, target): record}, align_statistics)"""
    p = _params(api, cs, lanes)
    db = _db(api, cs, lanes)
    q = api.Profiles([cs.entries[k] for k in keep], p) if isinstance(cs, sc.ProfileSet) else api.Queries([cs.queries[k] for k in keep], p)
    try:
        hits, off = _hit_lists(api, lists)
        api.prefilter_result_set(q, hits, off)
        alns, aoff = api.align(db, q, p)
        got = {}
        for i, k in enumerate(keep):
            for r in range(int(aoff[i]), int(aoff[i + 1])):
                a = alns[r]
                assert (k, int(a.db_key)) not in got, "two records for " + cs.describe(k, int(a.db_key))
                got[(k, int(a.db_key))] = (int(a.raw_score), int(a.q_start), int(a.q_end), int(a.db_start), int(a.db_end), int(a.q_len), int(a.db_len))
        return got, api.align_statistics(q)
    finally:
        q.close()


CONSISTENCY_REFUSALS = ("disagrees with the score pass", "Score of forward/backward SW differ")      # mk_align.hip: run_align_device


def _consistency_refusal(err):
    return any(text in str(err) for text in CONSISTENCY_REFUSALS)


def _run_stage(api, cs, lanes=(32, 16), max_rows=None, form="default"):
    """align on the case set's lists -> ({(query, target): (raw_score, q_start, q_end, db_start, db_end, q_len, db_len)}, align_statistics,
    the queries that took part)"""
    rows = cs.columns if isinstance(cs, sc.ProfileSet) else [len(s) for s in cs.queries]
    keep = [q for q in range(len(cs.lists)) if max_rows is None or rows[q] <= max_rows]
    try:
        got, stats = _align(api, cs, lanes, keep, [cs.lists[k] for k in keep])
    except api.MkError as err:
        # Only the stage's two consistency refusals (position pass against score pass, forward against reverse score) are narrowed: they come from
        # finished kernels whose results disagree, refuse the whole batch and name no pair.  Every other error -- a HIP error among them, which has
        # the same error code -- is raised at once, with no further GPU call.
        if not _consistency_refusal(err):
            raise
        found = []
        for k in keep:
            try:
                _align(api, cs, lanes, [k], [cs.lists[k]])
            except api.MkError as e1:
                if not _consistency_refusal(e1):
                    raise
                alone = []
                for t in cs.lists[k] if len(cs.lists[k]) <= 65 else []:
                    try:
                        _align(api, cs, lanes, [k], [[t]])
                    except api.MkError as e2:
                        if not _consistency_refusal(e2):
                            raise
                        alone.append(t)
                exp = cs.expected(lanes)
                for t in alone or cs.lists[k][:3]:
                    found.append("%s: oracle %s (score, q_end, t_end, q_start, t_start)%s"
                                 % (cs.describe(k, t), exp[(k, t)][:5], "" if alone else " -- the list is refused, none of its pairs alone"))
        raise AssertionError("[%s, lanes %s] the stage refused the batch: %s\n%d lists / pairs refused on their own:\n%s"
                             % (form, lanes, err, len(found), "\n".join(found[:12])))
    return got, stats, keep


def _check(cs, lanes, got, stats, keep, form):
    exp = cs.expected(lanes)
    profile = isinstance(cs, sc.ProfileSet)
    bad, n_pairs, n_records = [], 0, 0
    for k in keep:
        for t in cs.lists[k]:
            n_pairs += 1
            e = exp[(k, t)]
            assert e[5] == 0
            q_len = cs.columns[k] if profile else len(cs.queries[k])
            want = (e[0], e[3], e[1], e[4], e[2], q_len, len(cs.targets[t])) if e[0] > 0 else None
            n_records += want is not None
            if got.get((k, t)) != want:
                bad.append("%s [%s, lanes %s]: stage %s, oracle %s (raw_score, q_start, q_end, db_start, db_end, q_len, db_len)"
                           % (cs.describe(k, t), form, lanes, got.get((k, t)), want))
    assert not bad, "%d of %d pairs differ from the oracle:\n%s" % (len(bad), n_pairs, "\n".join(bad[:8]))
    assert len(got) == n_records
    assert stats["pairs_listed"] == n_pairs and stats["pairs_scored"] == stats["pairs_listed"], stats


def _stage_names(api):
    return {k for k in api.kernel_stats() if k.startswith("sw_")}


def _expected_launches(cs, exp, keep=None):
    """the per-tile kernel names a run over the case set must leave in kernel_stats()"""
    fwd, pos, rev = set(), set(), set()
    for q, t, _ in cs.pairs():
        if keep is not None and q not in keep:
            continue
        e = exp[(q, t)]
        rows = sc.TILE_ROWS[sc.tile_cfg(len(cs.queries[q]))]
        fwd.add("sw_fwd_rows%d" % rows)
        if e[0] > 0:
            pos.add("sw_pos_rows%d" % rows)
            rev.add("sw_rev_rows%d" % sc.TILE_ROWS[sc.tile_cfg(e[1] + 1)])       # a reverse job has the rows up to the end cell
    return fwd, pos, rev


# ---- sequence queries, in process (these switches are read per call) -----------------------------------------------------------------------
@pytest.mark.parametrize("name,lanes", GROUP_LANES)
def test_stage_equals_the_oracle(gpu_api, monkeypatch, name, lanes):
    for k in ("MK_SW_EARLY_EXIT", "MK_SW_MULTI", "MK_SW_NARROW", "MK_SW_TPOS"):
        monkeypatch.delenv(k, raising=False)
    cs = sc.group(name)
    gpu_api.kernel_stats(reset=True)
    got, stats, keep = _run_stage(gpu_api, cs, lanes)
    names = _stage_names(gpu_api)
    _check(cs, lanes, got, stats, keep, "default")
    fwd, pos, rev = _expected_launches(cs, cs.expected(lanes))
    assert fwd | pos | rev <= names, sorted((fwd | pos | rev) - names)
    if name == "G1":                                    # every tile configuration: score pass, position pass and (the "last rows" pairs) reverse pass
        for tag in ("sw_fwd", "sw_pos", "sw_rev"):
            assert {"%s_rows%d" % (tag, r) for r in sc.TILE_ROWS} <= names, sorted(names)


@pytest.mark.parametrize("name,lanes", GROUP_LANES)
def test_stage_without_the_early_exit_equals_the_oracle(gpu_api, monkeypatch, name, lanes):
    monkeypatch.setenv("MK_SW_EARLY_EXIT", "0")         # no bound from the score pass, no stop at the known score
    cs = sc.group(name)
    got, stats, keep = _run_stage(gpu_api, cs, lanes, form="MK_SW_EARLY_EXIT=0")
    _check(cs, lanes, got, stats, keep, "MK_SW_EARLY_EXIT=0")


@pytest.mark.parametrize("name,lanes", GROUP_LANES)
def test_sw_pairs_on_the_same_pairs(gpu_api, name, lanes):
    """the int32 wavefront behind mk_sw_pairs on the pairs of the lists: one table of expected values pins both"""
    api = gpu_api
    cs = sc.group(name)
    exp = cs.expected(lanes)
    p = _params(api, cs, lanes)
    q = api.Queries(cs.queries, p)
    pairs = [(a, b) for a, b, _ in cs.pairs()]
    try:
        got = api.sw_pairs(_db(api, cs, lanes), q, [a for a, _ in pairs], [b for _, b in pairs], with_start=True, params=p)
    finally:
        q.close()
    bad = []
    for k, (a, b) in enumerate(pairs):
        e, g = exp[(a, b)], tuple(int(x) for x in got[k])
        if (g != e[:5]) if e[0] > 0 else (g[0] != 0):
            bad.append("%s: sw_pairs %s, oracle %s (score, q_end, t_end, q_start, t_start)" % (cs.describe(a, b), g, e[:5]))
    assert not bad, "%d of %d pairs differ from the oracle:\n%s" % (len(bad), len(pairs), "\n".join(bad[:8]))


# ---- sequence queries, the forms fixed at a process's first call ----------------------------------------------------------------------------
def child_every_group(form):
    """(run in a child process with the switches of CHILD_FORMS[form] set) every sequence group under this form of the stage"""
    from metaeuk_amd import api
    api.init(0)
    multi = form == "multi"
    for name, lanes in GROUP_LANES:
        cs = sc.group(name)
        api.kernel_stats(reset=True)
        got, stats, keep = _run_stage(api, cs, lanes, max_rows=MULTI_MAX_ROWS if multi else None, form=form)
        names = _stage_names(api)
        _check(cs, lanes, got, stats, keep, form)
        if multi:
            assert len(keep) < len(cs.lists) or max(len(s) for s in cs.queries) <= MULTI_MAX_ROWS
            fwd, pos, rev = _expected_launches(cs, cs.expected(lanes), set(keep))
            classes = lambda tag, per_tile: {"%s_%s" % (tag, "rows32_64" if int(n.rsplit("rows", 1)[1]) <= 64 else
                                                        ("rows96_256" if int(n.rsplit("rows", 1)[1]) <= 256 else "rows384_1024")) for n in per_tile}
            assert classes("sw_pos", pos) | classes("sw_rev", rev) <= names, sorted(names)
            assert not [n for n in names if n.startswith(("sw_pos_rows", "sw_rev_rows")) and n.count("_") == 2], sorted(names)
            if name == "G1":
                assert {"%s_%s" % (tag, c) for tag in ("sw_pos", "sw_rev") for c in ("rows32_64", "rows96_256", "rows384_1024")} <= names, sorted(names)
    print("every group under %s: ok" % form)


@pytest.mark.parametrize("form", sorted(CHILD_FORMS))
def test_stage_forms_fixed_at_start_equal_the_oracle(form):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MK_SW_")}
    env.update(MK_DEBUG="1", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]), **CHILD_FORMS[form])
    r = subprocess.run([sys.executable, "-c", "import test_gpu_sw_kernels as t; t.child_every_group(%r)" % form], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "every group under %s: ok" % form in r.stdout, (r.stdout[-1000:], r.stderr[-6000:])


# ---- profile queries ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "MK_SW_EARLY_EXIT=0", "MK_SW_NARROW=0", "MK_SW_TPOS=0"])
def test_profile_stage_equals_the_oracle(gpu_api, monkeypatch, form):
    for k in ("MK_SW_EARLY_EXIT", "MK_SW_MULTI", "MK_SW_NARROW", "MK_SW_TPOS"):
        monkeypatch.delenv(k, raising=False)
    if form != "default":
        monkeypatch.setenv(*form.split("="))
    ps = sc.profile_group()
    gpu_api.kernel_stats(reset=True)
    got, stats, keep = _run_stage(gpu_api, ps, form=form)
    names = _stage_names(gpu_api)
    _check(ps, (32, 16), got, stats, keep, form)
    assert {"sw_fwd_rows512", "sw_fwd_rows768", "sw_fwd_rows1024"} <= names, sorted(names)
    transposed = {n for n in names if n.startswith("sw_pos_rows") and n.endswith("t")}
    if form in ("default", "MK_SW_EARLY_EXIT=0"):
        assert transposed == {"sw_pos_rows512t", "sw_pos_rows768t"}, sorted(names)
    else:
        assert not transposed, sorted(names)                                 # (MK_SW_NARROW=0 switches the transposed position pass off too)
