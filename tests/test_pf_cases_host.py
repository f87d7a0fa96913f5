"""Why tests/test_gpu_pf_cases.py cannot pass by accident (no GPU): the hits every case of tests/pf_cases.py REALLY gets -- enumerated from the
oracle's own pieces: its similar k-mer lists, its masked targets, a Python dictionary of the target k-mers -- are the designed ones; the
expected hit lists from the plain restatement of the rule (pf_cases.find_duplicates, first_best) and the oracle's diagonal scores are what the
oracle's pipeline prints (both of its paths, and the reference harness where it exists); five wrong rules each change a named case; the
groups are balanced and the coverage tables complete."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import pf_cases as pc

N_CASES = {"R12": 63, "R3": 120, "S": 224}         # literals: a case that vanishes from a builder is noticed here
SCORED_GROUPS = ("R12", "R3", "S")
POW = [20 ** p for p in range(6)]


class _Oracle:
    """the oracle's pieces, loaded once"""

    def __init__(self):
        L = self.L = oracle.lib()
        self.kmer_mat, self.ung_mat = oracle.submat(1, 8.0, -0.2), oracle.submat(0, 2.0, -0.2)
        L.mko_scoremat_build.restype = C.c_void_p
        L.mko_kmer_list6.restype = C.c_size_t
        self.three = C.c_void_p(L.mko_scoremat_build(C.byref(self.kmer_mat), C.c_int(3)))
        self.buf = np.zeros(1 << 20, dtype=np.uint64)

    def bias(self, codes):
        b = np.zeros(max(1, len(codes)), dtype=np.float32)
        self.L.mko_comp_bias(C.byref(self.kmer_mat), codes.ctypes.data_as(C.c_void_p), C.c_int(len(codes)), C.c_float(1.0), b.ctypes.data_as(C.c_void_p))
        return b

    def similar(self, codes, bias, i):
        """the similar k-mer list of query start i (mko_prefilter.c: seq_kmer_gen), None for a window with an X on a used position"""
        kmer = np.array([codes[i + p] for p in pc.SPACED], dtype=np.uint8)
        if (kmer == 20).any():
            return None
        corr = np.float32(0)
        for p in pc.SPACED:
            corr = np.float32(corr + bias[i + p])
        b = int(float(corr) - 0.5) if corr < 0 else int(float(corr) + 0.5)          # the cast to short truncates
        thr = max(pc.KMER_THR - b, 0)
        while True:
            n = self.L.mko_kmer_list6(self.three, kmer.ctypes.data_as(C.c_void_p), C.c_short(thr), self.buf.ctypes.data_as(C.c_void_p), C.c_size_t(self.buf.size))
            if n <= self.buf.size:
                return self.buf[:n].copy()
            self.buf = np.zeros(n, dtype=np.uint64)

    def masked(self, seq):
        codes = oracle.encode(seq).copy()
        self.L.mko_tantan_mask(C.byref(self.kmer_mat), codes.ctypes.data_as(C.c_void_p), C.c_int(len(seq)), C.c_double(float(np.float32(0.9))), C.c_int(4))
        return codes

    def profile(self, codes, bias):
        prof = np.zeros(len(codes) * 21, dtype=np.int8)
        self.L.mko_ungapped_profile(C.byref(self.ung_mat), codes.ctypes.data_as(C.c_void_p), C.c_int(len(codes)), bias.ctypes.data_as(C.c_void_p), prof.ctypes.data_as(C.c_void_p))
        return prof

    def score(self, prof, q_len, t_codes, d16):
        return int(self.L.mko_ungapped_score(prof.ctypes.data_as(C.c_void_p), C.c_int(q_len), t_codes.ctypes.data_as(C.c_void_p), C.c_int(len(t_codes)), C.c_uint16(d16)))


@pytest.fixture(scope="module")
def orc():
    return _Oracle()


class _Realised:
    """one group: masked targets, the dictionary of their k-mers, every query's hits per target in arrival order, the scores"""

    def __init__(self, orc, cs):
        self.cs, self.orc = cs, orc
        self.masked = [orc.masked(t) for t in cs.targets]
        index = {}                                                      # k-mer -> [(target, first position)], targets ascending
        for t, codes in enumerate(self.masked):
            seen = set()
            for i in range(len(codes) - pc.SPAN + 1):
                w = [int(codes[i + p]) for p in pc.SPACED]
                if 20 in w:
                    continue
                k = sum(c * f for c, f in zip(w, POW))
                if k not in seen:                                       # (self scores are at least 6 * 20 = 120: no k-mer is left out for its score)
                    seen.add(k)
                    index.setdefault(k, []).append((t, i))
        self.index = index
        self.index_keys = np.array(sorted(index), dtype=np.uint64)
        self.hits, self.prof, self._by_string = [], [], {}
        for s in cs.queries:
            if s not in self._by_string:
                self._by_string[s] = self._enumerate(s)
            self.hits.append(self._by_string[s][0])
            self.prof.append(self._by_string[s][1])

    def _enumerate(self, s):
        codes = oracle.encode(s)
        bias = self.orc.bias(codes)
        hits = {}
        for i in range(len(s) - pc.SPAN + 1):
            sim = self.orc.similar(codes, bias, i)
            if sim is None:
                continue
            for k in sim[np.isin(sim, self.index_keys)]:
                for t, pos in self.index[int(k)]:
                    hits.setdefault(t, []).append((i - pos) & 0xFFFF)
        return hits, self.orc.profile(codes, bias)

    def lines(self, q, rule=lambda hits: {t: pc.find_duplicates(h) for t, h in hits.items()}):
        """{target: (score printed, signed diagonal)} of query q; rule: {target: arrival sequence} -> {target: emitted}"""
        out = {}
        for t, emitted in rule(self.hits[q]).items():
            scores = [self.orc.score(self.prof[q], len(self.cs.queries[q]), self.masked[t], d) for d in emitted]
            k = pc.first_best(emitted, scores)
            if k is not None and min(255, scores[k]) >= pc.MIN_SCORE:
                out[t] = (scores[k], emitted[k] - 0x10000 if emitted[k] >= 0x8000 else emitted[k])
        return out

    def block(self, q):
        lines = self.lines(q)
        assert len(lines) < 300, "the --max-seqs cut is not part of these cases"
        return "".join("%d\t%d\t%d\n" % (t, s, d) for t, (s, d) in sorted(lines.items(), key=lambda kv: (-kv[1][0], kv[0])))


_REAL = {}


@pytest.fixture(scope="module")
def realised(orc):
    def get(name):
        if name not in _REAL:
            _REAL[name] = _Realised(orc, pc.group(name))
        return _REAL[name]
    return get


def _case_queries(cs):
    return sorted({c.q for c in cs.cases})


@pytest.mark.parametrize("name", SCORED_GROUPS)
def test_realised_hit_sequences(realised, name):
    """every case gets exactly its designed hits in the designed order -- no chance hit, no masked segment, no window across a separator --
    and a query with cases hits no target without a case"""
    cs, R = pc.group(name), realised(name)
    assert len(cs.cases) == N_CASES[name]
    for t, (seq, m) in enumerate(zip(cs.targets, R.masked)):
        assert bytes(m) == bytes(oracle.encode(seq)), "the repeat masker touched target %d of %s" % (t, name)
    bad = []
    for c in cs.cases:
        got = R.hits[c.q].get(c.t, [])
        if got != [d & 0xFFFF for d in c.hits]:
            bad.append("%s: realised %s" % (cs.describe(c.q, c.t), [d - 0x10000 if d >= 0x8000 else d for d in got]))
    assert not bad, "\n".join(bad[:10])
    for q in _case_queries(cs):
        stray = [t for t in R.hits[q] if (q, t) not in cs.by_pair]
        assert not stray, "query %d of %s: chance hits in targets %s" % (q, name, stray[:10])
    # the chains: as many k-mers as segments (no window across a separator is one)
    if name != "S":
        orc_ = R.orc
        for q in _case_queries(cs):
            codes = oracle.encode(cs.queries[q])
            starts = [i for i in range(len(codes) - pc.SPAN + 1) if orc_.similar(codes, orc_.bias(codes), i) is not None]
            assert starts == list(range(0, len(codes), pc.SPAN + pc.GAP)), (name, q)


@pytest.mark.parametrize("name", SCORED_GROUPS)
def test_expected_values_against_the_oracle(realised, name, tmp_path, monkeypatch):
    """find_duplicates + first_best + mko_ungapped_score on the realised hits give the block the oracle's pipeline prints -- presence, reported
    diagonal and pref_score -- on its literal path and on its device model, and the reference harness prints the same where it exists; every
    case's outcome is the one its label promises"""
    cs, R = pc.group(name), realised(name)
    opref, _ = oracle.run_pipeline(cs.targets, cs.queries, str(tmp_path / "literal"))
    monkeypatch.setenv("MKO_OVERFLOW_MODEL", "1")
    mpref, _ = oracle.run_pipeline(cs.targets, cs.queries, str(tmp_path / "model"))
    monkeypatch.delenv("MKO_OVERFLOW_MODEL")
    assert mpref == opref, "the oracle's device model differs from its literal path in queries %s" % [i for i in range(len(opref)) if opref[i] != mpref[i]]
    for q in _case_queries(cs):
        assert R.block(q) == opref[q], "query %d of %s:\nPython\n%soracle\n%s" % (q, name, R.block(q), opref[q])
    for c in cs.cases:
        line = R.lines(c.q).get(c.t)
        if c.expect == "absent":
            assert line is None, cs.describe(c.q, c.t)
        else:
            assert line is not None and (c.expect[1] is None or line[1] == c.expect[1]), (cs.describe(c.q, c.t), line)
    if os.path.exists(oracle.REF):
        rpref, _ = oracle.run_ref_pipeline(cs.targets, cs.queries, str(tmp_path / "ref"), extra=["--threads", "4"])
        assert rpref == opref


def test_the_saturated_case_saturates_twice(realised):
    """"255 twice": both emitted diagonals reach 255, the second scores higher, the first is reported with its exact score"""
    cs, R = pc.group("R12"), realised("R12")
    (c,) = [c for c in cs.cases if c.label.startswith("255 twice")]
    emitted = pc.find_duplicates(R.hits[c.q][c.t])
    scores = [R.orc.score(R.prof[c.q], len(cs.queries[c.q]), R.masked[c.t], d) for d in emitted]
    print("255 twice: emitted", emitted, "scores", scores)
    assert len(emitted) == 2 and 255 <= scores[0] < scores[1]
    assert R.lines(c.q)[c.t] == (scores[0], c.expect[1])


# ---- mutants of the rule -------------------------------------------------------------------------------------------------------------------
def _mutant(which):
    """a wrong rule over ONE QUERY's hits {target: arrival sequence} -> {target: emitted}"""
    def rule(hits):
        out, carry = {}, 0
        for t in sorted(hits):
            h = list(hits[t])
            if which == "M5":                                            # diagonal order instead of arrival order
                h.sort()
            key = (lambda d: d) if which == "M1" else (lambda d: d & 0xFF)      # M1: 16-bit diagonals
            kept, prev = [], carry if which == "M3" else 0               # M3: the previous target's last byte carries over
            for n, d in enumerate(h):
                if key(d) == prev and not (which == "M2" and n == 0):    # M2: a target's first hit is never kept
                    kept.append(d)
                prev = key(d)
            carry = prev
            emitted = []
            if kept:
                prev = key(kept[0]) + 1
                for d in kept:
                    if prev != key(d):
                        emitted.append(d)
                    prev = key(d)
            out[t] = emitted[:1] if which == "M4" else emitted           # M4: only the first kept hit of a target is emitted
        return out
    return rule


MUTANTS = {"M1": "compare 16-bit diagonals", "M2": "a target's first hit is never kept", "M3": "the previous target's last byte carries over",
           "M4": "only the first kept hit of a target is emitted", "M5": "hits in diagonal order instead of arrival order"}


def test_mutants_of_the_rule_change_named_cases(realised):
    """each wrong rule changes the expected line of at least one case; the table is printed"""
    table = {m: [] for m in MUTANTS}
    for name in SCORED_GROUPS:
        cs, R = pc.group(name), realised(name)
        for q in _case_queries(cs):
            right = R.lines(q)
            assert R.lines(q, rule=_mutant(None)) == right           # the scaffold of the mutants is the rule itself
            for m in MUTANTS:
                wrong = R.lines(q, rule=_mutant(m))
                for c in cs.cases:
                    if c.q == q and wrong.get(c.t) != right.get(c.t):
                        table[m].append("%s %s" % (c.group, c.label))
    for m, text in MUTANTS.items():
        labels = sorted(set(table[m]))
        print("%s (%s): %d cases -- %s" % (m, text, len(table[m]), "; ".join(labels[:12]) + (" ..." if len(labels) > 12 else "")))
    for m in MUTANTS:
        assert table[m], "no case separates %s (%s)" % (m, MUTANTS[m])
    # the patterns the issue names
    assert any("[d,d+256]" in l for l in table["M1"]) and any("lone 0" in l for l in table["M2"])
    assert any("boundary, right" in l for l in table["M3"]) and any("longer e" in l for l in table["M4"]) and any("[d,e,d,e]" in l for l in table["M5"])


# ---- balance and coverage ------------------------------------------------------------------------------------------------------------------
def test_groups_are_balanced_and_complete(tmp_path):
    for name in SCORED_GROUPS:
        cs = pc.group(name)
        for g in sorted({c.group for c in cs.cases}):
            kinds = {c.expect == "absent" for c in cs.cases if c.group == g}
            assert kinds == {True, False}, "group %s has only %s cases" % (g, "absent" if True in kinds else "present")
    r12 = pc.group("R12")
    for table in (pc.R1_SEQUENCES, pc.R2_SEQUENCES):
        for label, _, _ in table:
            assert any(c.label == label for c in r12.cases), "no chain holds " + label
    r3 = pc.group("R3")
    assert r3.by_pair[(0, 0)].label.startswith("first target") and r3.by_pair[(0, len(r3.targets) - 1)].label.startswith("last target")
    assert sum(1 for c in r3.cases if c.expect != "absent") >= 70 > 64          # more survivors than one wave of the sort
    pairs = {c.label: c.t for c in r3.cases if c.label.startswith("boundary")}
    for left, right in (("boundary, left [d,d]", "boundary, right lone d"), ("boundary, left [e,d,d]", "boundary, right lone 0"),
                        ("boundary, left [d,e]", "boundary, right lone e")):
        assert pairs[right] == pairs[left] + 1
        assert r3.by_pair[(0, pairs[left])].hits[-1] & 0xFF == r3.by_pair[(0, pairs[right])].hits[0] & 0xFF or "lone 0" in right
    # T: present and absent pairs by the oracle
    t = pc.group("T")
    opref, _ = oracle.run_pipeline(t.targets, t.queries, str(tmp_path))
    found = [{int(l.split("\t")[0]) for l in b.splitlines()} for b in opref]
    assert all(f for f in found) and all(len(f) < len(t.targets) for f in found)
    assert all(c.t in found[c.q] for c in t.cases), [t.describe(c.q, c.t) for c in t.cases if c.t not in found[c.q]]
    total_t = sum(len(pc.group(n).targets) for n in pc.GROUPS)
    total_q = sum(len(pc.group(n).queries) for n in pc.GROUPS)
    assert total_t <= 700 and total_q <= 120
    assert max(len(s) for n in pc.GROUPS for s in pc.group(n).queries + pc.group(n).targets) <= max(pc.tier_maxpos()) + 10


def test_coverage_tables():
    """S: every (query alignment, target alignment, overlap mod 4) on positive diagonals, every alignment pair on negative ones, from the
    cumulative lengths; T: exactly maxpos + 9 and maxpos + 10 residues for every limit of both tier sets"""
    s = pc.group("S")
    q_off = np.concatenate(([0], np.cumsum([len(x) for x in s.queries])))
    t_off = np.concatenate(([0], np.cumsum([len(x) for x in s.targets])))
    pos, neg = pc.scorer_coverage(s, q_off, t_off)
    assert pos == {(a, b, c) for a in range(4) for b in range(4) for c in range(4)}
    assert {(a, b) for a, b, _ in neg} == {(a, b) for a in range(4) for b in range(4)}
    for n in pc.S_LENGTHS:
        for m in range(4):
            assert any(c.label.startswith("S len %d p " % n) and c.hits[0] % 4 == m for c in s.cases), (n, m)
    for r in range(1, 5):
        assert any(c.label.endswith("r %d" % r) for c in s.cases)
    prod, mini = pc.tiers()
    assert [t[2] for t in prod] == [64, 128, 1024, 2048] and [t[2] for t in mini] == [32, 64, 64, 256]      # mk_prefilter.hip:1080-1082, :637, :656
    want = sorted(mp + k for mp in {t[2] for t in prod + mini} for k in (9, 10))
    assert sorted(len(x) for x in pc.group("T").queries) == want
    assert sorted(len(x) for x in pc.group("TL").queries) == want


def _similar_kmers(orc, s):
    """(k-mer starts, similar k-mers over all of them) of a query"""
    codes = oracle.encode(s)
    bias = orc.bias(codes)
    lists = [orc.similar(codes, bias, i) for i in range(len(s) - pc.SPAN + 1)]
    return sum(1 for l in lists if l is not None), sum(len(l) for l in lists if l is not None)


def test_tier_edge_queries_classify_by_their_length(orc, tmp_path):
    """TL: one k-mer and few enough similar k-mers that no limit[t] of either tier set can send a query on -- before the tiers have run on the
    database and after -- so maxpos[t] decides; the lone hit on diagonal 0 is realised and printed by the oracle; every tier that can be
    reached by length (and the global path behind the last) is where one query belongs and its sibling of one more k-mer start does not.
    TK: the two queries lie between limit[1] and limit[2] of the untouched miniature set, under 64 / at 65 k-mer starts"""
    prod, mini = pc.tiers()
    tl = pc.group("TL")
    R = _Realised(orc, tl)
    assert len(tl.cases) == 12 and len(tl.targets) == 12
    kms = []
    for c in tl.cases:
        starts, km = _similar_kmers(orc, tl.queries[c.q])
        print("%s: %d similar k-mers" % (c.label, km))
        assert starts == 1 and km > 0
        assert R.hits[c.q] == {c.t: [0]}, tl.describe(c.q, c.t)             # one index hit: a tier that ran this query measures 1 / km hits per similar k-mer
        kms.append(km)
    worst = max(pc.HPK_FRESH, 1.0 / min(kms))                               # the most hits per similar k-mer a tier can assume for this database
    print("TL: %d .. %d similar k-mers, smallest possible limit %.0f" % (min(kms), max(kms), min(pc.tier_limits(prod + mini, worst))))
    assert max(kms) <= pc.TL_KMERS_MOST and max(kms) < min(pc.tier_limits(prod + mini, worst))
    opref, _ = oracle.run_pipeline(tl.targets, tl.queries, str(tmp_path / "tl"))
    for c in tl.cases:
        assert R.block(c.q) == opref[c.q] and [int(l.split("\t")[0]) for l in opref[c.q].splitlines()] == [c.t], tl.describe(c.q, c.t)
    # tier -> where the query of one more k-mer start goes (None: the global path).  64 starts are the second miniature tier's, 65 the fourth's:
    # the third is TK's
    for tier_set, behind in ((prod, {0: 1, 1: 2, 2: 3, 3: None}), (mini, {0: 1, 1: 3, 3: None})):
        for t, nxt in behind.items():
            assert pc.tier_by_length(tier_set, tier_set[t][2]) == t and pc.tier_by_length(tier_set, tier_set[t][2] + 1) == nxt
    tk = pc.group("TK")
    assert len(tk.targets) != len(tl.targets)                               # another database: the sizing the tiers learned on TL is dropped
    lim = pc.tier_limits(mini, pc.HPK_FRESH)
    npos = []
    for q, s in enumerate(tk.queries):
        starts, km = _similar_kmers(orc, s)
        print("TK query %d: %d residues, %d k-mers, %d similar k-mers between %.0f and %.0f" % (q, len(s), starts, km, lim[1], lim[2]))
        assert 1.05 * lim[1] < km < 0.95 * lim[2] and km < lim[3]
        npos.append(len(s) - 9)
    assert npos == [mini[2][2], mini[2][2] + 1] and mini[1][2] == mini[2][2] < mini[3][2]
    opref, _ = oracle.run_pipeline(tk.targets, tk.queries, str(tmp_path / "tk"))
    found = [{int(l.split("\t")[0]) for l in b.splitlines()} for b in opref]
    assert all(c.t in found[c.q] for c in tk.cases) and all(len(f) < len(tk.targets) for f in found)
