"""--alt-ali on the GPU: mk_alt_alignments (mk_altali.hip) against its host twin, record for record, on the planted set of test_altali_host.py,
and against the ordinary stage: round r of a chain equals mk_align over a second database with the chain's mask written into the residues."""
import subprocess

import numpy as np
import pytest

from test_altali_host import FLAGS, params_of, workload

pytestmark = pytest.mark.gpu
FIELDS = ("db_key", "bit_score", "seq_id", "qcov", "dbcov", "evalue", "q_start", "q_end", "q_len", "db_start", "db_end", "db_len", "aln_len", "raw_score")
rec = lambda a: tuple(getattr(a, f) for f in FIELDS)
order = lambda r: (r[5], -r[1], r[11], r[0])                 # Matcher::compareHits: e-value, bit score, db_len, key; sorted() is stable


def aligned(api, targets_res, flags):
    """(db, batch) of the planted set over the given target residues, aligned by the ordinary stage; the lists as plain records"""
    queries, targets, lists = workload()
    t_off = np.concatenate([[0], np.cumsum([len(t) for t in targets])]).astype(np.uint64)
    db = api.TargetDB.sequences(targets_res, t_off)
    q = api.Queries(list(queries))
    hits = np.zeros(sum(len(l) for l in lists), dtype=api.HIT_DTYPE)
    hits["seq_id"] = [t for l in lists for t in l]
    api.prefilter_result_set(q, hits, np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64))
    alns, off = api.align(db, q, params_of(api, flags))
    return db, q, [[rec(alns[k]) for k in range(int(off[i]), int(off[i + 1]))] for i in range(q.n)]


@pytest.fixture(scope="module")
def planted(gpu_api):
    queries, targets, lists = workload()
    res, t_off = gpu_api.encode(list(targets))
    return res[:int(t_off[-1])], t_off


def twin_chains(api, planted, q, origins, flags, n):
    """per query and origin: [origin record, alternatives of the host twin in round order]"""
    (res, t_off), bias, out = planted, q.derived()[2], []
    for qi, recs in enumerate(origins):
        lo, hi = int(q.off[qi]), int(q.off[qi + 1])
        out.append([])
        for r in recs:
            alts = api.alt_alignments_host(q.res[lo:hi], bias[lo:hi], res[int(t_off[r[0]]):int(t_off[r[0] + 1])], api.Alignment(*r), int(t_off[-1]), params_of(api, flags), n)
            out[-1].append([r] + [rec(a) for a in alts])
    return out


@pytest.mark.parametrize("flags,n", [("e001", 1), ("e001", 2), ("e001", 5), ("open", 3), ("c05 id03", 2)])
def test_kernel_equals_host_twin(gpu_api, planted, flags, n):
    api, (db, q, origins) = gpu_api, aligned(gpu_api, planted[0], flags)
    assert sum(len(o) for o in origins) >= 14 and origins[-1] == []
    chains = twin_chains(api, planted, q, origins, flags, n)
    api.kernel_stats(reset=True)
    alns, off = api.alt_alignments(db, q, n, params_of(api, flags))
    got = [[rec(alns[k]) for k in range(int(off[i]), int(off[i + 1]))] for i in range(q.n)]
    want = [sorted([r for c in cs for r in c], key=order) for cs in chains]
    assert got == want
    assert api.kernel_stats(reset=True)["alt_alignments"]["cells"] > 10000
    if flags == "e001" and n == 5:
        assert [len(c) for c in chains[0]] == [3, 3]         # the repeat's two origins: two alternatives each, a rejection ends both before 5
    if flags == "open":
        w = [c for cs in chains for c in cs if c[0][8] == 1][0]
        assert len(w) == n + 1 and w[1:] == [w[0]] * n       # the empty mask of a one-column origin: the same record N more times


def test_rounds_equal_the_ordinary_stage_on_hand_masked_targets(gpu_api, planted):      # (one origin per target: the queries behind the repeat)
    api, (res, t_off) = gpu_api, planted
    db, q, origins = aligned(api, res, "e001")
    chains = twin_chains(api, planted, q, origins, "e001", 3)
    masked = np.array(res)
    for r in range(1, 4):
        for cs in chains[1:]:
            for c in cs:
                if len(c) >= r:                              # the mask of the chain in front of round r: the record accepted last
                    masked[int(t_off[c[r - 1][0]]) + c[r - 1][9]:int(t_off[c[r - 1][0]]) + c[r - 1][10]] = 20
        _, _, again = aligned(api, masked, "e001")
        for qi in range(1, q.n):
            assert sorted(again[qi], key=order) == sorted([c[r] for c in chains[qi] if len(c) > r], key=order), (r, qi)


def test_alt_ali_0_and_refusals_by_name(gpu_api, planted):
    from test_gpu_profile import _golden_inputs
    api, p = gpu_api, params_of(gpu_api, "e001")
    db, q, _ = aligned(api, planted[0], "e001")
    api.kernel_stats(reset=True)
    alns, off = api.align(db, q, p)
    before = (bytes(alns), bytes(off))
    alns, off = api.alt_alignments(db, q, 0, p)              # no alternatives asked for: the result untouched, nothing of the stage launched
    assert (bytes(alns), bytes(off)) == before and not [k for k in api.kernel_stats() if k.startswith("alt_alignments")]
    with pytest.raises(api.MkError, match="error -1.*--alt-ali -1"):
        api.alt_alignments(db, q, -1, p)
    with pytest.raises(api.MkError, match="error -3.*--alt-ali 33"):
        api.alt_alignments(db, q, 33, p)
    for field, value in (("alignment_mode", 3), ("add_backtrace", 1)):
        bad = params_of(api, "e001")
        setattr(bad, field, value)
        with pytest.raises(api.MkError, match="error -3.*--alt-ali with --alignment-mode 3 / -a"):
            api.alt_alignments(db, q, 1, bad)
    with pytest.raises(api.MkError, match="error -1.*no alignment result"):
        api.alt_alignments(db, api.Queries(["ACDEFGHIKLMNP"]), 1, p)
    with pytest.raises(api.MkError, match="error -3.*profile"):
        api.alt_alignments(db, api.Profiles(_golden_inputs()[1][:1]), 1, p)


def test_command_equals_the_library(gpu_api, planted, tmp_path):
    from metaeuk_amd import build
    from test_gpu_backtrace import _read_result_db, _write_seq_db
    api, t = gpu_api, str(tmp_path) + "/"
    queries, targets, lists = workload()
    _write_seq_db(t + "targets", targets); _write_seq_db(t + "queries", queries)
    off = 0
    with open(t + "pref", "wb") as d, open(t + "pref.index", "w") as i:
        for k, l in enumerate(lists):
            body = "".join("%d\t0\t0\n" % x for x in l).encode() + b"\0"
            d.write(body); i.write("%d\t%d\t%d\n" % (k, off, len(body))); off += len(body)
    open(t + "pref.dbtype", "wb").write((7).to_bytes(4, "little"))
    cmd = [build.BIN, "align", t + "queries", t + "targets", t + "pref", t + "aln", "--alignment-mode", "2", "-e", "0.001", "--min-aln-len", "5", "--threads", "4"]
    subprocess.check_call(cmd + ["--alt-ali", "2"], stderr=subprocess.DEVNULL, timeout=120)
    db, q, _ = aligned(api, planted[0], "e001")
    alns, aoff = api.alt_alignments(db, q, 2, params_of(api, "e001"))
    assert [_read_result_db(t + "aln")[k] for k in range(q.n)] == [api.format_alignments(alns, int(aoff[k]), int(aoff[k + 1])) for k in range(q.n)]
    for bad in (cmd[:5] + [t + "bad"] + cmd[6:] + ["--alt-ali", "2", "-a", "1"],
                [build.BIN, "predictexons", t + "queries", t + "targets", t + "bad", t + "tmp", "--alt-ali", "1"]):
        r = subprocess.run(bad, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode != 0 and b"--alt-ali" in r.stderr and not (tmp_path / "bad.dbtype").exists(), (bad, r.stderr[-300:])
