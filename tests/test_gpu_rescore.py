"""rescorediagonal --rescore-mode 2 on the GPU: mk_rescore_diagonal (mk_rescore.hip) against its host twin, record for record, on a seeded set with
the tie and reset cases planted across lane and sweep boundaries; the command and `search --alignment-mode 4` against the real binary's three runs."""
import subprocess

import numpy as np
import pytest

from test_backtrace_host import _blocks, _lines, _text
from test_rescore_host import FIXTURES, cell, fixture_params, mat

pytestmark = pytest.mark.gpu
FIELDS = ("db_key", "bit_score", "seq_id", "qcov", "dbcov", "evalue", "q_start", "q_end", "q_len", "db_start", "db_end", "db_len", "aln_len", "raw_score")
FLAGS = {"no filter": dict(evalue_thr=1e9, add_backtrace=1), "c05 id03": FIXTURES["e2e_process_rescore_c05_id03.txt.gz"][0]}


@pytest.fixture(scope="module")
def seeded(gpu_api):
    """(db, batch with hand-placed prefilter lists, {flags: per query the host twin's kept records in list order})"""
    api, rs = gpu_api, np.random.RandomState(11)
    W, S = api.RESCORE_SEG, api.RESCORE_GROUP * api.RESCORE_SEG                    # cells per lane and per sweep
    targets = [rs.randint(0, 20, int(n)).astype(np.uint8) for n in rs.randint(140, 400, 300)] + [rs.randint(0, 20, 70000).astype(np.uint8)]
    queries, lists = [], []
    # aligned lengths 1 .. 5, S - 1, S, S + 1, 2 S - 1, 2 S + 1: the query lies inside the target, the diagonal is as long as the query
    for k, n in enumerate([1, 2, 3, 4, 5, S - 1, S, S + 1, 2 * S - 1, 2 * S + 1]):
        queries.append(np.array(targets[k][7 + k:7 + k + n])); lists.append([(k, -(7 + k))])
    # ties and resets across a lane boundary (cell W) and a sweep boundary (cell S) on an otherwise negative diagonal; no positive cell at all
    patterns = [p for b in (W, S) for p in ({b - 2: 4, b - 1: 4, b: -4, b + 1: -4, b + 2: 4, b + 3: 4},      # two equal maxima: the first wins
                                            {b - 1: 4, b: -4, b + 1: 5, b + 2: 5},                              # the sum touches 0: the latest reset starts
                                            {b - 3: 4, b - 2: -4, b - 1: 4, b: -4, b + 1: 9},                   # two resets around the boundary
                                            {0: 9, b - 1: 4, b: 5}, {2 * S: 9})] + [{}]                          # maximum at 0 / across / at the last cell
    for k, pattern in enumerate(patterns):
        q = rs.randint(0, 20, 2 * S + 1).astype(np.uint8)
        for pos in range(2 * S + 1):
            q[pos], targets[30 + k][3 + pos] = cell(pattern.get(pos, -1))
        queries.append(q); lists.append([(30 + k, -3)])
    # mutated fragments on their own diagonal and on random ones of both signs; a query without a hit; one with more pairs than a workgroup takes
    for k in range(170):
        t, n = int(rs.randint(100, 300)), int(rs.randint(20, 120))
        lo = int(rs.randint(0, len(targets[t]) - n))
        f = np.array(targets[t][lo:lo + n])
        f[rs.rand(n) < 0.15] = rs.randint(0, 20)
        queries.append(f); lists.append([(t, -lo)] + [(int(u), int(rs.randint(-100, n))) for u in rs.randint(100, 300, int(rs.randint(0, 6)))])
    queries.append(rs.randint(0, 20, 50).astype(np.uint8)); lists.append([])
    queries.append(rs.randint(0, 20, 90).astype(np.uint8)); lists.append([(int(u), int(rs.randint(-100, 90))) for u in rs.randint(100, 300, 100)])
    # the long pair: diagonal 65436 stands for -100 (walked first, weak match) and -65636 (walked second, strong match)
    ql = rs.randint(0, 20, 120).astype(np.uint8)
    ql[5:25] = targets[300][105:125]; ql[40:100] = targets[300][65676:65736]
    queries.append(ql); lists.append([(300, 65436)])
    q_off, t_off, h_off = (np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.uint64) for xs in (queries, targets, lists))
    flat = [h for l in lists for h in l]
    hits = np.zeros(len(flat), dtype=api.HIT_DTYPE)
    hits["seq_id"] = [h[0] for h in flat]; hits["diagonal"] = [h[1] & 0xFFFF for h in flat]
    # all 16 combinations of (query start, target start) mod 4 in the buffers the kernel reads (diagonals of this set are their own signed value)
    assert len({((int(q_off[qi]) + max(d, 0)) % 4, (int(t_off[t]) + max(-d, 0)) % 4) for qi, l in enumerate(lists) for t, d in l if d < 32768}) == 16
    db = api.TargetDB.sequences(np.concatenate(targets), t_off)
    q = api.Queries.from_codes(np.concatenate(queries), q_off)
    api.prefilter_result_set(q, hits, h_off)
    want = {}
    for name, flags in FLAGS.items():
        p = fixture_params(api, flags)
        twin = [[api.rescore_diagonal_host(queries[qi], targets[t], d & 0xFFFF, int(t_off[-1]), p, mat=mat()) + (t,) for t, d in l] for qi, l in enumerate(lists)]
        want[name] = [[(t,) + tuple(getattr(a, f) for f in FIELDS[1:]) + (ids,) for kept, a, ids, t in l if kept] for l in twin]
    assert sum(len(w) for w in want["no filter"]) == len(flat) and len(flat) > 600
    return db, q, want


@pytest.mark.parametrize("sort", [0, 1])
@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_kernel_equals_host_twin(gpu_api, seeded, flags, sort):
    api, (db, q, want) = gpu_api, seeded
    alns, off = api.rescore_diagonal(db, q, fixture_params(api, FLAGS[flags]), sort_results=sort)
    ids = api.align_backtrace(q, len(alns))[2] if FLAGS[flags].get("add_backtrace") else None      # (-a: the identities, record by record)
    bad = []
    for qi, w in enumerate(want[flags]):
        w = sorted(w, key=lambda r: (r[5], -r[1], r[11], r[0])) if sort else w          # Matcher::compareHits: e-value, bit score, db_len, key
        got = [tuple(getattr(alns[k], f) for f in FIELDS) + (w[k - int(off[qi])][-1] if ids is None else int(ids[k]),) for k in range(int(off[qi]), int(off[qi + 1]))]
        if got != w:
            bad.append((qi, got[:2], w[:2]))
    assert not bad, (len(bad), bad[:2])
    assert api.kernel_stats(reset=True)["rescore_diagonal"]["cells"] > 10000


def test_refusals_by_name(gpu_api, seeded):
    from test_gpu_profile import _golden_inputs
    api, (db, q, _) = gpu_api, seeded
    for mode in (0, 1, 3, 4):
        with pytest.raises(api.MkError, match="error -3.*--rescore-mode %d" % mode):
            api.rescore_diagonal(db, q, rescore_mode=mode)
    hit = np.zeros(1, dtype=api.HIT_DTYPE)
    hit["seq_id"], hit["diagonal"] = 5, 1000                   # 1000 >= the query's 40 residues, and -64536 misses the target
    for batch, want in ((api.Queries.from_codes(np.zeros(40, np.uint8), np.array([0, 40], dtype=np.uint64)), "error -1.*diagonal"),
                        (api.Profiles(_golden_inputs()[1][:1]), "error -3.*profile")):
        api.prefilter_result_set(batch, hit, np.array([0, 1], dtype=np.uint64))
        with pytest.raises(api.MkError, match=want):
            api.rescore_diagonal(db, batch)


def test_commands_reproduce_the_real_rescorediagonal(gpu_api, tmp_path):
    """over the real process's pref_0, and `search --alignment-mode 4` over its own prefilter, which equals that pref_0; refusals by name"""
    from metaeuk_amd import build
    from test_gpu_backtrace import L2, _read_result_db, _write_seq_db
    t = str(tmp_path) + "/"
    frags = [l.rsplit("\t", 1)[1] for l in _lines("e2e_process_orfs.txt.gz")]
    _write_seq_db(t + "targets", _lines("e2e_targets.txt.gz")); _write_seq_db(t + "aa_6f", frags)
    pref, off = _blocks(_text("e2e_process_pref.txt.gz")), 0
    with open(t + "pref_0", "wb") as d, open(t + "pref_0.index", "w") as i:
        for k in range(len(frags)):
            body = "".join(ln + "\n" for ln in pref.get(k, [])).encode() + b"\0"
            d.write(body); i.write("%d\t%d\t%d\n" % (k, off, len(body))); off += len(body)
    open(t + "pref_0.dbtype", "wb").write((7).to_bytes(4, "little"))
    resc = [build.BIN, "rescorediagonal", t + "aa_6f", t + "targets", t + "pref_0"]
    for n, (name, (_, argv)) in enumerate(sorted(FIXTURES.items())):
        subprocess.check_call(resc + [t + "resc%d" % n, "--rescore-mode", "2", "--threads", "4"] + argv, stderr=subprocess.DEVNULL, timeout=120)
        db = _read_result_db(t + "resc%d" % n)
        assert "".join(">%d\n%s" % (k, db[k]) for k in sorted(db)) == _text(name), name
        subprocess.check_call([build.BIN, "search", t + "aa_6f", t + "targets", t + "srch%d" % n, t + "tmp", "-s", "5.7", "--alignment-mode", "4", "--threads", "4",
                               "--ref-l2-bytes", str(L2)] + argv, stderr=subprocess.DEVNULL, timeout=120)
        assert open(t + "srch%d" % n, "rb").read() == open(t + "resc%d" % n, "rb").read(), name
    assert open(t + "resc0.dbtype", "rb").read() == (5).to_bytes(4, "little")
    for bad in (["--rescore-mode", "0"], ["--rescore-mode", "1"], ["--rescore-mode", "3"], ["--rescore-mode", "4"], ["--rescore-mode", "2", "--filter-hits", "1"],
                ["--rescore-mode", "2", "--wrapped-scoring", "1"], ["--rescore-mode", "2", "--include-identity", "1"]):
        r = subprocess.run(resc + [t + "bad"] + bad, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode != 0 and bad[-2].encode() in r.stderr, (bad, r.stderr[-300:])
    # one DB on both sides (the identity rule), under another spelling of its path, in the command and in the search
    for same in (resc[:3] + [t + "./aa_6f", t + "pref_0", t + "bad", "--rescore-mode", "2"],
                 [build.BIN, "search", t + "aa_6f", t + "./aa_6f", t + "bad", t + "tmp", "--alignment-mode", "4"]):
        r = subprocess.run(same, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode != 0 and b"query DB as the target DB" in r.stderr, (same, r.stderr[-300:])
