"""The hand-made Smith-Waterman cases of tests/sw_cases.py against the reference alone (no GPU): the textbook Gotoh recurrence equals the
oracle's striped passes -- the claim in the header of metaeuk_amd/csrc/mk_sw.hip, stated as a test -- and the cases are what they were built
to be (ties are ties, end cells lie where the groups want them, every tile configuration and list size is there), so that the GPU tests
of tests/test_gpu_sw_kernels.py cannot pass on cases that have lost their edge."""
import pytest

import oracle
import sw_cases as sc


@pytest.fixture(scope="module", params=sorted(sc.SEQUENCE_GROUPS))
def cases(request):
    return sc.group(request.param)


def test_no_reverse_mismatch_and_positive_scores(cases):
    zero = 0
    for lanes in sc.lanes_of(cases.name):
        for (q, t), e in cases.expected(lanes).items():
            assert e[5] == 0, cases.describe(q, t)
            if cases.name != "G5":
                assert e[0] > 0, (cases.describe(q, t), e)
            elif e[0] == 0:
                zero += 1
            else:
                assert e[1] >= e[3] >= 0 and e[2] >= e[4] >= 0, (cases.describe(q, t), e)
    if cases.name == "G5":
        scores = [e[0] for e in cases.expected().values()]
        assert zero >= 5 and sum(1 for s in scores if 1 <= s <= 3) >= 3, scores
        assert sum(1 for q, t, _ in cases.pairs() if len(cases.targets[t]) == 1) >= 3
        # the GPU test has no record for the pairs without a score, and for no other: they are the poly-W queries' pairs
        assert zero == sum(1 for _, _, label in cases.pairs() if label.startswith("G5/poly-W")) == 36


def test_lists_name_no_target_twice(cases):
    for q, l in enumerate(cases.lists):
        assert len(set(l)) == len(l) and l, q
        assert all(0 <= t < len(cases.targets) for t in l)


def test_textbook_gotoh_equals_the_striped_reference(cases):
    """score, first column, smallest row: cell by cell the same DP for every SIMD width.  A disagreement here is a finding against the
    kernels' recurrence (plain Gotoh), not against this test."""
    every = cases.name in ("G4", "G5")
    checked = 0
    for q, t, label in cases.pairs():
        if not (every or sc.small(cases, q, t)):
            continue
        g = sc.gotoh(cases.queries[q], cases.targets[t], cases.gap_open, cases.gap_extend, cases.bias_scale)
        for lanes in sc.lanes_of(cases.name):
            e = cases.expected(lanes)[(q, t)]
            if e[0] == 0:
                assert g.score == 0, (cases.describe(q, t), lanes, g, e)
            else:
                assert (g.score, g.min_row, g.first_col) == e[:3], (cases.describe(q, t), lanes, g, e)
            checked += 1
    assert checked >= {"G1": 50, "G2": 60, "G3": 2000, "G4": 2 * 190, "G5": 40, "G6": 4}[cases.name], checked


def test_ties_are_ties():
    cs = sc.group("G4")
    seen = {"a": 0, "b": 0, "c": 0, "d": 0}
    for q, t, label in cs.pairs():
        kind = label.split("/")[1][0]
        if kind == "e":
            continue
        g = sc.gotoh(cs.queries[q], cs.targets[t], cs.gap_open, cs.gap_extend, cs.bias_scale)
        m = len(cs.queries[q])
        if kind == "a":
            assert g.cols_at_max >= 2 and g.first_col == m - 1, (label, g)                     # the end of the FIRST copy
        elif kind == "b":
            assert g.cols_at_max == 1 and g.first_col == len(cs.targets[t]) - 1, (label, g)    # the maximum rises in the second copy
        else:
            assert g.rows_at_max >= 2, (label, g)
        seen[kind] += 1
    assert seen == {"a": 25, "b": 25, "c": 25, "d": 4}, seen
    # (d): both rows of the tie belong to one lane (R rows per lane: 12 on the 192-row tile, 2 / 3 / 4 on the 32- / 48- / 64-row tiles)
    for q, t, label in cs.pairs():
        if label.startswith("G4/d"):
            L = len(cs.queries[q])
            R = {30: 2, 45: 3, 60: 4, 160: 12}[L]
            e = cs.expected()[(q, t)]
            rows = (2, 10) if L == 160 else (4, 5)
            assert e[1] == rows[0] and rows[0] // R == rows[1] // R, (label, e)


def test_tile_edge_cases_end_where_they_should():
    for cs in (sc.group("G1"), sc.group("G6")):
        for q, t, label in cs.pairs():
            e = cs.expected()[(q, t)]
            L = len(cs.queries[q])
            if label.endswith(("/last rows", "/copy", "/second copy")):
                assert e[1] == L - 1, (cs.describe(q, t), e)
        assert sorted({len(s) for s in cs.queries}) == sorted(sc.G1_LENGTHS if cs.name == "G1" else sc.G6_LENGTHS)


def test_column_edge_cases_end_where_they_should():
    cs = sc.group("G2")
    assert [len(s) for s in cs.queries] == list(sc.G2_QUERIES)
    for q, l in enumerate(cs.lists):
        for kind in ("G2/last column", "G2/early column"):
            assert sorted(len(cs.targets[t]) for t, label in zip(l, cs.labels[q]) if label == kind) == sorted(sc.G2_TARGETS)
        assert cs.labels[q].count("G2/block edge") >= 8
    for q, t, label in cs.pairs():
        e = cs.expected()[(q, t)]
        n = len(cs.targets[t])
        if label == "G2/last column":
            assert e[2] == n - 1, (cs.describe(q, t), e)
        elif label == "G2/early column":
            assert 0 <= e[2] <= 15, (cs.describe(q, t), e)
        else:
            QL = len(cs.queries[q])
            lane = (QL - 1) // sc.SCORE_ROWS_PER_LANE[sc.tile_cfg(QL)]
            assert e[1] == QL - 1 and (e[2] + lane) % 16 == 15 and e[2] < n - 1, (cs.describe(q, t), e)


def test_every_tile_configuration_and_list_size_is_there():
    per_cfg = [0] * len(sc.TILE_ROWS)
    for name in sc.SEQUENCE_GROUPS:
        cs = sc.group(name)
        for q, t, _ in cs.pairs():
            per_cfg[sc.tile_cfg(len(cs.queries[q]))] += 1
    assert min(per_cfg) >= 5, per_cfg
    g3 = sc.group("G3")
    sizes = sorted(len(l) for l in g3.lists)
    assert sizes == sorted(list(sc.G3_SIZES) * 2 + list(sc.G3_LARGE) + [2, 2, 2]), sizes
    assert sorted({len(s) for s in g3.queries}) == [40, 60, 400]
    two = [sorted(len(g3.targets[t]) for t in l) for q, l in enumerate(g3.lists) if g3.labels[q][0].startswith("G3/two")]
    assert two == [[1, 300], [16, 17], [20, 300]], two
    pool = {t for q, l in enumerate(g3.lists) if len(l) >= 2048 for t in l}
    assert all(20 <= len(g3.targets[t]) <= 40 for t in pool)
    # the survivors of the group on tiles of at most 64 rows (one align call, one launch per tile): no multiple of the 8 jobs of a wave
    survivors = sum(1 for (q, t), e in g3.expected().items() if len(g3.queries[q]) <= 64 and e[0] > 0)
    assert survivors % 8 != 0, survivors


def test_profile_cases():
    ps = sc.profile_group()
    assert sorted(set(ps.columns)) == sorted(sc.P_COLUMNS)
    assert [sc.tile_cfg(c) for c in sc.P_COLUMNS] == [8, 9, 10]
    assert {len(l) for l in ps.lists} == set(sc.P_SIZES)
    frag_lens = {len(ps.targets[t]) for _, t, _ in ps.pairs()}
    assert frag_lens == set(sc.P_FRAGMENTS)
    exp = ps.expected()
    for (q, t), e in exp.items():
        assert e[5] == 0 and e[0] > 0, (ps.describe(q, t), e)
    for q, l in enumerate(ps.lists):
        assert len(set(l)) == len(l)
    mixed = [l for q, l in enumerate(ps.lists) if "257 among short" in ps.labels[q][0]]
    assert len(mixed) == 4 and all(sorted(len(ps.targets[t]) for t in l)[-2:][0] <= 128 for l in mixed)
    # The favoured scores of ~120 are 30 per row of the alignment profile (int8 score / 4, at most 31): the 300-residue consensus fragment scores
    # ~ 9000 -- beyond the byte pass (the oracle reruns it in words) and beyond the stage's e-value table, but 520 rows x 31 cannot reach the
    # 32767 at which the word pass saturates; no profile of a packed tile (at most 768 rows) can, and no sequence query either (a row scores at
    # most the matrix maximum of 22 plus its int8 bias).  The saturating add of swp_kernel's SAT branch is therefore never observable: there is
    # no missing case to look for, a plain add in its place computes the same on every valid input.
    hot = [e for (q, t), e in exp.items() if ps.labels[q][0].endswith("consensus 300")]
    assert len(hot) == 1 and 8000 < hot[0][0] <= 300 * 31, hot
