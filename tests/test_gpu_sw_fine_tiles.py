"""The packed score pass (mk_sw.hip: swp_kernel) around its finer bodies: 80 and 112 rows inside the 96- and 128-row launches (sequence
queries of 65 .. 80 and 97 .. 112 residues).  Queries on both sides of every edge, each against related and unrelated targets whose lengths
put the step count on both sides of half a block of 16 steps (where the DP's last steps fall in the unrolled block); every pair must give the oracle's
(score, q_start, q_end, db_start, db_end), and the stage with MK_SW_FINE=0 (a child process: the switch is read once) the same records, the same
formatted alignments and as many of them.  (The library reports no name for the body a wave ran: that the two forms differ rests on the switch
being honoured by mk_align.hip; what guards the new bodies themselves is the oracle in the default form.)"""
import json
import os
import random
import subprocess
import sys

import pytest

import sw_cases as sc
import test_gpu_sw_kernels as k

pytestmark = pytest.mark.gpu
# 64 | 65: the 64- and the 96-row launch; 80 | 81: the body of 5 and of 6 rows per lane; 96 | 97: the 128-row launch; 112 | 113: 7 and 8 rows per
# lane; 128: the last query of that launch; 48: a launch without a finer body (3 of 4 slots per lane: the other place where a slot's row depends on the rows per lane), as a control
QUERY_LENGTHS = (48, 64, 65, 79, 80, 81, 96, 97, 111, 112, 113, 128)
# a 16-lane group runs tLen + 15 steps in unrolled blocks of 16: (tLen + 15) mod 16 = 0, 1, 7, 8, 9 and 15 -- the DP's last step at the block's
# edge, one step into the next block, and on both sides of its middle
TARGET_RESIDUES = (1, 2, 8, 9, 10, 0)
TARGET_BASES = (32, 64, 96, 112)
SHORT_TARGETS = (17, 25, 57)                # with the 24 others: 27 pairs per query = three waves of 8 jobs and one of 3


def _fit(rng, s, n):
    """s cut or flanked to exactly n residues"""
    if len(s) >= n:
        a = rng.randrange(len(s) - n + 1)
        return s[a:a + n]
    left = rng.randrange(n - len(s) + 1)
    return sc._rand(rng, left) + s + sc._rand(rng, n - len(s) - left)


def fine_tile_cases():
    cs = sc.CaseSet("fine")
    lengths = [b + r if r else b + 16 for b in TARGET_BASES for r in TARGET_RESIDUES] + list(SHORT_TARGETS)
    assert {(t + 15) % 16 for t in lengths} >= {0, 1, 7, 8, 9, 15} and len(lengths) == 27
    for L in QUERY_LENGTHS:
        rng = random.Random(7000 + L)
        base = sc._rand(rng, L)
        q = cs.query(base)
        order = lengths[:]
        rng.shuffle(order)                   # neighbours of different length: the two halves of a packed pair
        for n, t_len in enumerate(order):
            if n % 3 == 2:
                cs.pair(q, sc._rand(rng, t_len), "fine/random %d" % t_len)
            elif n % 3 == 1:
                cs.pair(q, _fit(rng, sc._mutate(rng, base, 0.15, 0.06), t_len), "fine/indels %d" % t_len)
            else:
                cs.pair(q, _fit(rng, base, t_len), "fine/copy %d" % t_len)
    return cs


_CASES = []


def _cases():
    if not _CASES:
        _CASES.append(fine_tile_cases())
    return _CASES[0]


def _stage(api):
    """the stage on the case set -> (records {(q, t): tuple}, statistics, queries, the formatted alignments per query, alignments per query)"""
    cs = _cases()
    got, stats, keep = k._run_stage(api, cs)
    p = k._params(api, cs)
    q = api.Queries(cs.queries, p)
    try:
        hits, off = k._hit_lists(api, cs.lists)
        api.prefilter_result_set(q, hits, off)
        alns, aoff = api.align(k._db(api, cs, (32, 16)), q, p)
        text = [api.format_alignments(alns, int(aoff[i]), int(aoff[i + 1])) for i in range(len(cs.queries))]
        counts = [int(aoff[i + 1]) - int(aoff[i]) for i in range(len(cs.queries))]
    finally:
        q.close()
    return got, stats, keep, text, counts


def child_records():
    """(run in a child process with MK_DEBUG=1 MK_SW_FINE=0) the stage's records as one JSON line"""
    from metaeuk_amd import api
    api.init(0)
    cs = _cases()
    got, stats, keep, text, counts = _stage(api)
    k._check(cs, (32, 16), got, stats, keep, "MK_SW_FINE=0")
    text = [t.decode("latin-1") if isinstance(t, bytes) else t for t in text]
    print("RECORDS " + json.dumps({"got": sorted([list(key) + list(v) for key, v in got.items()]), "text": text, "counts": counts}))


def test_case_set_covers_what_it_names():
    cs = _cases()
    assert sorted(len(s) for s in cs.queries) == sorted(QUERY_LENGTHS)
    for q, l in enumerate(cs.lists):
        assert len(l) % 8 == 3                                                   # a last wave of fewer than 8 jobs
        assert {(len(cs.targets[t]) + 15) % 16 for t in l} >= {0, 1, 7, 8, 9, 15}
        assert len({len(cs.targets[t]) for t in l}) == len(l)                     # whichever two targets share a lane group differ in length
    exp = cs.expected()
    positive = sum(1 for v in exp.values() if v[0] > 0)
    assert positive >= len(exp) // 2                                             # the related targets are found, so position and reverse passes run


def test_fine_tiles_equal_the_oracle_and_the_coarse_form(gpu_api, monkeypatch):
    for name in ("MK_SW_FINE", "MK_SW_EARLY_EXIT", "MK_SW_MULTI", "MK_SW_NARROW", "MK_SW_TPOS"):
        monkeypatch.delenv(name, raising=False)
    cs = _cases()
    gpu_api.kernel_stats(reset=True)
    got, stats, keep, text, counts = _stage(gpu_api)
    names = k._stage_names(gpu_api)
    k._check(cs, (32, 16), got, stats, keep, "default")
    assert {"sw_fwd_rows48", "sw_fwd_rows64", "sw_fwd_rows96", "sw_fwd_rows128"} <= names, sorted(names)

    here = os.path.dirname(os.path.abspath(__file__))
    env = {key: v for key, v in os.environ.items() if not key.startswith("MK_SW_")}
    env.update(MK_DEBUG="1", MK_SW_FINE="0", PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_sw_fine_tiles as t; t.child_records()"], env=env, capture_output=True, text=True,
                       timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RECORDS ")]
    assert r.returncode == 0 and len(lines) == 1, (r.stdout[-1000:], r.stderr[-6000:])
    coarse = json.loads(lines[0][len("RECORDS "):])
    text = [t.decode("latin-1") if isinstance(t, bytes) else t for t in text]
    assert counts == coarse["counts"]
    assert sorted([list(key) + list(v) for key, v in got.items()]) == coarse["got"]
    assert text == coarse["text"]
