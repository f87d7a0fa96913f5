"""mk_profile_backtrace (trace_profile_kernel, mk_trace.hip) against its host twin, record by record, behind gappedprefilter + align of golden profiles."""
import numpy as np
import pytest

from test_gpu_profile import _golden_inputs
from test_gpu_ungapped_prefilter import _offsets
from test_gpu_ungapped_profile import _params

pytestmark = pytest.mark.gpu


def _aligned(api, entries, targets):
    """every profile against every target, every positive score kept -> (db, batch, params, records, offsets, [(ops, identities, attempts)] by the twin)"""
    p = _params(api, max_seqs=max(300, len(targets)), min_ungapped_score=0, evalue_thr=1.7976931348623157e308, min_aln_len=0)
    db, q = api.TargetDB.sequences(np.concatenate(targets), _offsets(targets), p), api.Profiles(entries, p)
    api.gapped_prefilter_profile(db, q, p)
    alns, aoff = api.align(db, q, p)
    recs, (letters, _, aln32, _), own = np.frombuffer(alns, dtype=np.dtype(api.Alignment)).copy(), q.derived(), lambda a, i: a[int(q.off[i]):int(q.off[i + 1])]
    twin = [api.backtrace_profile_host(own(aln32, i), own(letters, i), int(r["q_start"]), int(r["q_end"] - r["q_start"]) + 1,
                                       targets[int(r["db_key"])][int(r["db_start"]):int(r["db_end"]) + 1], int(r["raw_score"]))
            for i in range(q.n) for r in recs[int(aoff[i]):int(aoff[i + 1])]]
    return db, q, p, recs, np.array(aoff), twin


@pytest.fixture(scope="module")
def world(gpu_api):
    """six golden profiles, one that scores in ONE column (W in column 9: records of one column x one residue) and one that scores nowhere; 200 targets
    cut from the golden consensus with mutations, indels and flanks: 70 from the first profile (more than one 64-lane run), one that needs three bands"""
    rs, flat = np.random.RandomState(61), bytes([0xEC] * 20 + [0, 0, 10, 0, 0])
    entries = list(_golden_inputs()[1][:6])
    cons = [np.frombuffer(e[:-1], dtype=np.int8).reshape(-1, 25)[:, :20].argmax(axis=1).astype(np.uint8) for e in entries]
    entries += [flat * 9 + bytes([0xEC] * 18 + [100, 0xEC, 18, 18, 10, 0, 0]) + flat * 10 + b"\0", flat * 30 + b"\0"]
    targets, rnd = [], lambda n: rs.randint(0, 20, int(n)).astype(np.uint8)
    for k in range(199):
        c = cons[0] if k < 70 else cons[1 + k % 5]
        a, n = int(rs.randint(0, len(c) - 60)), int(rs.randint(25, 60))
        piece = np.array(c[a:a + n])
        piece[rs.rand(n) < 0.1] = rs.randint(0, 20)
        if k % 3 == 0:                                                   # a deleted or an inserted stretch of 1 .. 3
            d, at = int(rs.randint(1, 4)), n // 2
            piece = np.concatenate([piece[:at], piece[at + d:]]) if k % 2 else np.concatenate([piece[:at], rnd(d), piece[at:]])
        targets.append(np.concatenate([rnd(rs.randint(0, 6)), piece, rnd(rs.randint(0, 6))]))
    c = cons[2][10:70]                                                   # equal spans with a 4-column and a 4-residue gap: first band 1
    targets.append(np.concatenate([c[:15], c[19:40], rnd(4), c[40:]]))
    db, q, p, recs, aoff, twin = w = _aligned(gpu_api, entries, targets)
    assert aoff[1] >= 65 and aoff[8] == aoff[7] and max(t[2] for t in twin) >= 3 and all(t[0] for t in twin)
    assert aoff[7] > aoff[6] and all(r["q_start"] == r["q_end"] == 9 and r["db_start"] == r["db_end"] for r in recs[int(aoff[6]):int(aoff[7])])
    return w + (np.array(gpu_api.prefilter_result(q)[0]),)


@pytest.mark.parametrize("mode,keep", [(0, True), (1, True), (2, False)])
def test_records_equal_the_twin(gpu_api, world, mode, keep):
    api, (db, q, p, recs, aoff, twin, hits) = gpu_api, world
    (alns, off2), (ops, ops_off, ids) = api.profile_backtrace(db, q, p, seq_id_mode=mode, keep_ops=keep)
    got = np.frombuffer(alns, dtype=np.dtype(api.Alignment))
    assert np.array_equal(off2, aoff) and np.array_equal(np.array(api.prefilter_result(q)[0]), hits)         # hits, record set and order: untouched
    assert all(np.array_equal(got[f], recs[f]) for f in recs.dtype.names if f not in ("aln_len", "seq_id"))
    den = [lambda r, n: n, lambda r, n: min(r["q_len"], r["db_len"]), lambda r, n: max(r["q_len"], r["db_len"])][mode]
    want = [(o if keep else b"", i, len(o), np.float32(i) / np.float32(den(r, len(o)))) for r, (o, i, _) in zip(recs, twin)]
    have = [(ops[int(ops_off[k]):int(ops_off[k + 1])], int(ids[k]), int(got["aln_len"][k]), np.float32(got["seq_id"][k])) for k in range(len(twin))]
    assert len(have) == len(recs) and not [(k, h, w) for k, (h, w) in enumerate(zip(have, want)) if h != w][:3]


@pytest.mark.parametrize("over", [0, 1])
def test_window_at_and_beyond_the_image(gpu_api, over):
    """capacity + 1 columns; two targets, the first 40 consensus residues and the 40 that end on column capacity (+ 1): a window the largest image holds / one beyond"""
    api, cap = gpu_api, gpu_api.PROFILE_TRACE_IMAGE_COLS
    cols = np.frombuffer(b"".join(e[:-1] for e in _golden_inputs()[1])[:(cap + 1) * 25], dtype=np.int8).reshape(cap + 1, 25).copy()
    cols[:40, :20] = cols[:40, 19::-1]                                   # (the golden profiles are alike: the first columns must score nowhere else)
    cons, cols = cols[:, :20].argmax(axis=1).astype(np.uint8), cols.tobytes()
    head, tail = cons[:40], cons[cap + over - 40:cap + over]
    db, q, p, recs, aoff, twin = _aligned(api, [cols + b"\0"], [np.concatenate([head[:20], head[22:]]), np.concatenate([tail[:18], [7, 7], tail[18:]])])
    assert len(recs) == 2 and int(recs["q_end"].max()) - int(recs["q_start"].min()) + 1 == cap + over and all(b"I" in t[0] or b"D" in t[0] for t in twin)
    api.kernel_stats(reset=True)
    _, (ops, ops_off, ids) = api.profile_backtrace(db, q, p)
    assert [ops[int(ops_off[k]):int(ops_off[k + 1])] for k in range(2)] == [t[0] for t in twin] and list(ids) == [t[1] for t in twin]
    st = api.kernel_stats(reset=True)
    assert [name for name in st if name.startswith("trace_profile") and st[name]["cells"] > 0] == ["trace_profile_global" if over else "trace_profile"]


def test_refusals(gpu_api, world):
    """a sequence batch; a profile batch without an alignment result; arguments out of range"""
    api, (db, q, p) = gpu_api, world[:3]
    seqs, fresh = api.Queries.from_codes(np.arange(20, dtype=np.uint8), _offsets([np.arange(20)])), api.Profiles(list(_golden_inputs()[1][:1]), p)
    for batch, kw, msg in ((seqs, {}, "error -3.*profile"), (fresh, {}, "error -1"), (q, dict(seq_id_mode=3), "error -1"), (q, dict(keep_ops=2), "error -1")):
        with pytest.raises(api.MkError, match=msg):
            api.profile_backtrace(db, batch, p, **kw)
