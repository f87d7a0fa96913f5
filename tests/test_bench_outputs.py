"""bench.py --dump-outputs: the sample of the last timed step's results that two builds are compared by."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("totals", "sample_queries", "hit_counts", "alignment_counts", "hits", "alignments")


def _load(d):
    out = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in NAMES)
    assert all(a.dtype == np.float64 for a in out.values())
    return out


def _fake_results(n, seed):
    from metaeuk_amd import api
    rng = np.random.default_rng(seed)
    hoff = np.zeros(n + 1, dtype=np.uint64)
    hoff[1:] = np.cumsum(rng.integers(0, 9, n))
    aoff = np.zeros(n + 1, dtype=np.uint64)
    aoff[1:] = np.cumsum(rng.integers(0, 3, n))
    hits = np.zeros(int(hoff[-1]), dtype=api.HIT_DTYPE)
    hits["seq_id"] = rng.integers(0, 2 ** 32, hits.size, dtype=np.uint64)
    hits["pref_score"] = rng.integers(-5, 300, hits.size)
    hits["diagonal"] = rng.integers(0, 65536, hits.size)
    alns = (api.Alignment * int(aoff[-1]))()
    view = np.frombuffer(alns, dtype=np.dtype(api.Alignment))
    for f in view.dtype.names:
        view[f] = rng.integers(0, 1000, view.size)
    view["evalue"] = rng.random(view.size) * 1e-30
    return hits, hoff, alns, aoff, view


def test_dump_outputs_sample(tmp_path, monkeypatch):
    """the records of the sampled queries, whole and in query order; the same sample from the same seed; a smaller one when the budget is short"""
    import bench
    from metaeuk_amd import api
    n = 1000
    hits, hoff, alns, aoff, view = _fake_results(n, 3)
    monkeypatch.setattr(bench, "DUMP_QUERIES", 256)
    bench.dump_outputs(api, str(tmp_path / "a"), hits, hoff, alns, aoff, seed=11)
    a = _load(str(tmp_path / "a"))
    assert a["totals"].tolist() == [n, int(hoff[-1]), int(aoff[-1])]
    take = a["sample_queries"].astype(np.int64)
    assert take.size == 256 and np.all(np.diff(take) > 0)
    assert a["hit_counts"].tolist() == np.diff(hoff.astype(np.int64))[take].tolist()
    assert a["alignment_counts"].tolist() == np.diff(aoff.astype(np.int64))[take].tolist()
    exp_h = np.concatenate([np.arange(int(hoff[q]), int(hoff[q + 1])) for q in take])
    exp_a = np.concatenate([np.arange(int(aoff[q]), int(aoff[q + 1])) for q in take])
    assert a["hits"].shape == (exp_h.size, 3) and a["alignments"].shape == (exp_a.size, len(view.dtype.names))
    for c, f in enumerate(("seq_id", "pref_score", "diagonal")):
        assert np.array_equal(a["hits"][:, c], hits[f][exp_h].astype(np.float64))
    for c, f in enumerate(view.dtype.names):
        assert np.array_equal(a["alignments"][:, c], view[f][exp_a].astype(np.float64))
    # the sample is a function of the seed and the number of queries alone
    bench.dump_outputs(api, str(tmp_path / "b"), hits, hoff, alns, aoff, seed=11)
    b = _load(str(tmp_path / "b"))
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)
    bench.dump_outputs(api, str(tmp_path / "c"), hits, hoff, alns, aoff, seed=12)
    assert not np.array_equal(_load(str(tmp_path / "c"))["sample_queries"], a["sample_queries"])
    # a budget the 256 queries' records do not fit: the sample is halved until they do
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20000)
    bench.dump_outputs(api, str(tmp_path / "d"), hits, hoff, alns, aoff, seed=11)
    d = _load(str(tmp_path / "d"))
    assert d["sample_queries"].size in (128, 64, 32, 16)
    assert sum(v.nbytes for k, v in d.items() if k != "totals") <= 20000
    assert set(d["sample_queries"].tolist()) <= set(a["sample_queries"].tolist())
    # no results at all
    e = np.zeros(5, dtype=np.uint64)
    bench.dump_outputs(api, str(tmp_path / "e"), np.zeros(0, dtype=api.HIT_DTYPE), e, (api.Alignment * 0)(), e, seed=11)
    z = _load(str(tmp_path / "e"))
    assert z["hits"].shape == (0, 3) and z["alignments"].shape[0] == 0 and z["totals"].tolist() == [4, 0, 0]


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path, gpu_api):
    """a plain run on a small workload: --steps sets the timed steps, the line carries ms_per_step and none of the --full legs, and the dump holds
    what a search of the same inputs returns"""
    import bench
    api = gpu_api
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--contigs", "30", "--targets", "400",
           "--dump-outputs", str(tmp_path / "o")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "fragments/s" and line["higher_is_better"] is True
    assert line["steps_with_other_counts"] == 0
    nq = _n_queries(line)
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - nq) < 1e-6 * nq        # value = fragments per second of one timed step
    for leg in ("cpu_baseline", "result_digest", "config4_profile_targets", "end_to_end_predictexons", "config5_60M"):
        assert leg not in line
    assert line["blocking"] is None
    d = _load(str(tmp_path / "o"))
    # the same inputs through the library here
    targets, queries, _ = bench.make_inputs(30, 400, 11, 0)
    t_res, t_off = bench.pack(targets)
    q_res, q_off = bench.pack(queries)
    params = api.default_params()
    params.host_l2_bytes = _host_l2()                      # as bench.py sets it
    db = api.TargetDB.from_codes(t_res, t_off, params)
    q = api.Queries.from_codes(q_res, q_off, params)
    (hits, hoff), (alns, aoff) = api.search(db, q)
    assert d["totals"].tolist() == [len(queries), int(hoff[-1]), int(aoff[-1])] == [len(queries), line["prefilter_hits"], line["alignments_passed"]]
    assert int(hoff[-1]) > 0 and int(aoff[-1]) > 0
    bench.dump_outputs(api, str(tmp_path / "here"), hits, hoff, alns, aoff, 11)
    here = _load(str(tmp_path / "here"))
    for k in NAMES:
        assert np.array_equal(d[k], here[k]), k
    q.close()
    db.close()


def _n_queries(line):
    import re
    return int(re.search(r"\((\d+) ORF fragments/rank", line["config"]["workload"]).group(1))


def _host_l2():
    import ctypes
    l2 = ctypes.CDLL(None).sysconf(191)
    return l2 if l2 and l2 > 0 else 262144
