"""Hand-made prefilter cases (tests/test_pf_cases_host.py, tests/test_gpu_pf_cases.py): planted 10-residue segments whose index hits arrive in a
designed order on designed diagonals, so that every branch of the double-diagonal rule (CacheFriendlyOperations::findDuplicates), every
(alignment, tail) shape of the dword scorer of diag_score_kernel and every k-mer-start limit of the per-query tiers is named and met -- as
targets, queries and a label for every (query, target) case.  Deterministic (seeded).  find_duplicates() and first_best() are the plain
restatement of the rule the device copies claim to equal.  No GPU and no fixtures here.

The construction: a query is a chain of distinct random segments of 10 residues -- the span of the k = 6 pattern 1101010011 -- separated by
XXX.  The don't-care positions of the pattern come in runs of at most two, so every window that touches a separator has an X on a used
position and is no k-mer: a chain of n segments has exactly n k-mers.  A target is X filler with copies of chosen segments at chosen
offsets; segment k of the query (at p_k) copied to u_k gives one hit on diagonal p_k - u_k, and the hits of a target arrive in query
order.  No segment is planted twice in a target (the index keeps a k-mer's first position per target only)."""
import os
import random
import re
from collections import namedtuple

import numpy as np

import oracle

AA = "ACDEFGHIKLMNPQRSTVWY"
SPACED = (0, 1, 3, 5, 8, 9)                 # used positions of 1101010011
SPAN = 10
GAP = 3                                     # X between the segments of a chain and between the copies in a target
KMER_THR = 112                              # int(163.2 - 5.7 * 8.917): the default sensitivity
MIN_SCORE = 15                              # --min-ungapped-score
SELF_FLOOR, CHANCE_CEILING = 140, 80        # a segment's k-mer scores >= 140 with itself and <= 80 with every other segment of its group:
                                            # the composition bias moves the threshold of 112 by far less than 28
EXTEND = GAP + 6                            # "the longer planted run": the copy goes on through the separator and six residues into the next segment
SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metaeuk_amd", "csrc", "mk_prefilter.hip")

Case = namedtuple("Case", "group label q t hits expect")
# hits: the designed arrival sequence of the target's hits (signed diagonals); expect: "absent", ("present", None) or ("present", diagonal)


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------
def find_duplicates(hits):
    """CacheFriendlyOperations::findDuplicates (computeTotalScore == false) on ONE target's hits in arrival order; hits: 16-bit diagonals
    (or tuples that start with one) -> the emitted ones, in order.  Pass 1 keeps a hit whose low diagonal byte equals the byte of the
    target's previous hit (0 before the first).  Pass 2 walks the kept hits with the byte of the first kept one plus 1 as predecessor and
    emits a hit whose byte differs from the previous kept hit's."""
    lo = lambda h: (h[0] if isinstance(h, tuple) else h) & 0xFF
    kept, prev = [], 0
    for h in hits:
        if lo(h) == prev:
            kept.append(h)
        prev = lo(h)
    out = []
    if kept:
        prev = (lo(kept[0]) + 1) & 0xFF
        for h in kept:
            if prev != lo(h):
                out.append(h)
            prev = lo(h)
    return out


def first_best(candidates, scores):
    """keepMaxScoreElementOnly on one target's scored candidates: the scores are clamped at 255, the FIRST candidate with the largest clamped
    score stays -> its index (None without candidates)"""
    if not candidates:
        return None
    clamped = [min(255, s) for s in scores]
    return clamped.index(max(clamped))


# ---- the tiers, read from the source -------------------------------------------------------------------------------------------------------
def tiers():
    """(production, miniature): four (cap, waves, maxpos, wgPerCu) each, from TIERS of mk_prefilter.hip (:1080-1082) with MK_STREAM_MAXPOS_A
    (:637), MK_STREAM_MAXPOS_B (:656) and the other MK_STREAM_* defaults resolved"""
    src = open(SOURCE).read()
    defs = {}
    for name, val in re.findall(r"#define (MK_STREAM_\w+) (\d+)", src):
        defs.setdefault(name, int(val))
    body = re.search(r"const FusedTier TIERS\[2 \* N_TIERS\] = \{(.*?)\};", src, re.S).group(1)
    rows = [tuple(int(defs.get(x.strip(), x.strip())) for x in r.split(",")) for r in re.findall(r"\{([^{}]*)\}", body)]
    assert len(rows) == 8 and rows[2][2] == defs["MK_STREAM_MAXPOS_A"] and rows[3][2] == defs["MK_STREAM_MAXPOS_B"]
    return rows[:4], rows[4:]


def tier_kernel_name(cap):
    """the name the per-query launch of a tier is booked under, from the snprintf that makes it (mk_prefilter.hip:2856)"""
    fmt = re.search(r'snprintf\(nm, sizeof\(nm\), "(\w+%d)", tiers\[t\]\.cap\)', open(SOURCE).read()).group(1)
    return fmt % cap


def global_kernel_name():
    """the global path books its copy of the rule as (mk_prefilter.hip:2293)"""
    return re.search(r'tb\("(double_hit)"', open(SOURCE).read()).group(1)


# ---- building blocks -----------------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return "".join(rng.choice(AA) for _ in range(n))


def _mutate(rng, s, rate):
    return "".join(rng.choice(AA) if rng.random() < rate else ch for ch in s)


_KMER_MAT = None


def _kmer_matrix():
    global _KMER_MAT
    if _KMER_MAT is None:
        m = oracle.submat(1, 8.0, -0.2)                                # the seed matrix of the k-mer lists
        _KMER_MAT = np.array([[m.sub[i][j] for j in range(20)] for i in range(20)], dtype=np.int32)
    return _KMER_MAT


def segments(rng, n):
    """n random 10-residue segments no two of which can be similar k-mers of each other"""
    M = _kmer_matrix()
    segs, codes = [], np.zeros((0, 6), dtype=np.int64)
    while len(segs) < n:
        s = _rand(rng, SPAN)
        c = np.array([AA.index(s[p]) for p in SPACED])
        if M[c, c].sum() < SELF_FLOOR or (len(segs) and M[codes, c].sum(axis=1).max() > CHANCE_CEILING):
            continue
        segs.append(s)
        codes = np.vstack([codes, c])
    return segs


class Chain:
    """segments joined by XXX; pos[k]: where segment k starts"""

    def __init__(self, segs):
        self.segs = list(segs)
        self.pos = [k * (SPAN + GAP) for k in range(len(segs))]
        self.seq = ("X" * GAP).join(segs)


def plant(chain, runs, tail=0):
    """a target for `chain` from the requested diagonal sequence.  runs: (diagonal, n, extend[, skip]) in arrival order -- n neighbouring
    segments copied as one piece (separators included) onto `diagonal`, `extend` more query residues behind the last one, `skip` segments
    left out in front.  A piece takes the next segments at which it lies inside the target and at least GAP away from every other piece
    -> (target, [diagonal of every hit in arrival order]) or None when the chain has too few segments"""
    placed, pieces, hits, k = [], [], [], 0
    for run in runs:
        d, n, ext = run[:3]
        k += run[3] if len(run) > 3 else 0
        while True:
            if k + n > len(chain.segs) or chain.pos[k + n - 1] + SPAN + ext > len(chain.seq):
                return None
            a, b = chain.pos[k], chain.pos[k + n - 1] + SPAN + ext
            u = a - d
            if u >= 0 and all(u >= e + GAP or u + (b - a) + GAP <= s for s, e in placed):
                break
            k += 1
        placed.append((u, u + b - a))
        pieces.append(chain.seq[a:b])
        hits += [d] * n
        k += n
    out = ["X"] * (max(e for _, e in placed) + tail)
    for (u, e), piece in zip(placed, pieces):
        assert all(ch == "X" for ch in out[u:e]), "planted pieces overlap"
        out[u:e] = piece
    return "".join(out), hits


class CaseSet:
    def __init__(self, name):
        self.name, self.targets, self.queries, self.cases = name, [], [], []
        self.by_pair = {}

    def query(self, s):
        self.queries.append(s)
        return len(self.queries) - 1

    def target(self, s):
        self.targets.append(s)
        return len(self.targets) - 1

    def case(self, group, label, q, t, hits, expect):
        c = Case(group, label, q, t, list(hits), expect)
        assert (q, t) not in self.by_pair
        self.cases.append(c)
        self.by_pair[(q, t)] = c
        return c

    def describe(self, q, t):
        c = self.by_pair.get((q, t))
        if c is None:
            return "%s: query %d x target %d (no designed hit)" % (self.name, q, t)
        return "%s %s: query %d (%d residues) x target %d (%d residues), designed hits %s" % (
            self.name, c.label, q, len(self.queries[q]), t, len(self.targets[t]), c.hits)


# ---- R1 / R2: the rule and the byte --------------------------------------------------------------------------------------------------------
def _sym(runs, d, e):
    val = {"d": d, "e": e, "d+256": d + 256}
    return [(val.get(r[0], r[0]),) + tuple(r[1:]) for r in runs]


# (label, runs with the diagonals d / e / d+256 or a number, expectation with the diagonal that is reported)
R1_SEQUENCES = (
    ("[d]", [("d", 1, 0)], "absent"),
    ("[d,e]", [("d", 1, 0), ("e", 1, 0)], "absent"),
    ("[d,e,d]", [("d", 1, 0), ("e", 1, 0), ("d", 1, 0)], "absent"),
    ("[d,e,d,e]", [("d", 1, 0), ("e", 1, 0), ("d", 1, 0), ("e", 1, 0)], "absent"),
    ("[d,d]", [("d", 2, 0)], ("present", "d")),
    ("[d,d,d]", [("d", 3, 0)], ("present", "d")),
    ("[d,d,d,d]", [("d", 4, 0)], ("present", "d")),
    ("[d,d,e]", [("d", 2, 0), ("e", 1, 0)], ("present", "d")),
    ("[e,d,d]", [("e", 1, 0), ("d", 2, 0)], ("present", "d")),
    ("[d,d,e,e] longer e", [("d", 2, 0), ("e", 2, EXTEND)], ("present", "e")),
    ("[d,d,e,e,d,d]", [("d", 2, 0), ("e", 2, 0), ("d", 2, 0)], ("present", None)),
    ("[d,d,e,d,d]", [("d", 2, 0), ("e", 1, 0), ("d", 2, 0)], ("present", "d")),
    ("255 twice, the second longer", [("d", 7, 0), ("e", 8, EXTEND)], ("present", "d")),
)
R2_SEQUENCES = (
    ("lone 0", [(0, 1, 0)], ("present", 0)),
    ("lone +256", [(256, 1, 0)], ("present", 256)),
    ("lone -256", [(-256, 1, 0)], ("present", -256)),
    ("lone 1", [(1, 1, 0)], "absent"),
    ("[d,d+256]", [("d", 1, 0), ("d+256", 1, 0)], ("present", "d+256")),
    ("[d+256,d]", [("d+256", 1, 0), ("d", 1, 0)], ("present", "d")),
    ("[d,d+256,d+256]", [("d", 1, 0), ("d+256", 2, 0)], ("present", "d+256")),
    ("[-3,-3]", [(-3, 2, 0)], ("present", -3)),
    ("[-3,253]", [(-3, 1, 0), (253, 1, 0)], ("present", 253)),
    ("[0,e,e] e better", [(0, 1, 0), ("e", 2, 0)], ("present", "e")),
    # one hit on 0 whose copy runs on through nine residues of the next segment (which is not planted again: the repeat masker would take it),
    # the two on e far apart: each scores as one segment
    ("[0,e,e] 0 better", [(0, 1, GAP + 9), ("e", 1, 0, 1), ("e", 1, 0, 5)], ("present", 0)),
)
# the chains of R1 + R2: (segments, d, e).  Their k-mer starts (length - 9) are 14, 53, 118 and 521: the first three tiers of the production
# set (64, 128, 1024) and tiers of 32, 64 and 256 of the miniature set; the last is beyond the miniature set (the global path behind it)
R12_CHAINS = ((2, -7, -40), (5, -7, -40), (10, 6, -27), (41, 47, 9))
# which chain carries which sequence decides the tier a sequence is tested in: the sequences a chain is too short for, by its number of
# segments (the chain of 41 carries all of them).  _add_sequences holds the builder to this table in both directions
_NEEDS_256 = ("255 twice, the second longer", "lone +256", "[d,d+256]", "[d+256,d]", "[d,d+256,d+256]", "[-3,253]")
R12_NOT_CARRIED = {
    2: ("[d,e,d]", "[d,e,d,e]", "[d,d,d]", "[d,d,d,d]", "[d,d,e]", "[e,d,d]", "[d,d,e,e] longer e", "[d,d,e,e,d,d]", "[d,d,e,d,d]",
        "[0,e,e] e better", "[0,e,e] 0 better") + _NEEDS_256,
    5: ("[e,d,d]", "[d,d,e,e,d,d]", "[d,d,e,d,d]", "[0,e,e] 0 better") + _NEEDS_256,
    10: _NEEDS_256,
    41: (),
}


def _add_sequences(cs, group, q, chain, table, d, e, tails):
    left_out = R12_NOT_CARRIED[len(chain.segs)]
    for label, runs, expect in table:
        got = plant(chain, _sym(runs, d, e), tail=next(tails))
        assert (got is None) == (label in left_out), "R12_NOT_CARRIED is wrong about %r on the chain of %d segments" % (label, len(chain.segs))
        if got is None:
            continue
        target, hits = got
        if expect != "absent":
            rep = expect[1]
            expect = ("present", {"d": d, "e": e, "d+256": d + 256}.get(rep, rep))
        cs.case(group, label, q, cs.target(target), hits, expect)


def _tails(rng):
    while True:
        yield rng.randrange(0, 4)                                        # X behind the last piece: the targets' offsets take every value mod 4


def rule_and_byte():
    cs = CaseSet("R12")
    rng = random.Random(8100)
    pool = segments(rng, sum(n for n, _, _ in R12_CHAINS))
    tails = _tails(rng)
    for n, d, e in R12_CHAINS:
        chain, pool = Chain(pool[:n]), pool[n:]
        q = cs.query(chain.seq)
        _add_sequences(cs, "R1", q, chain, R1_SEQUENCES, d, e, tails)
        _add_sequences(cs, "R2", q, chain, R2_SEQUENCES, d, e, tails)
    return cs


# ---- R3: run boundaries ---------------------------------------------------------------------------------------------------------------------
R3_HUB = ("[d,d]", "[d]", "[d,d,e]", "[d,e]", "[e,d,d]", "[d,d,d]", "[d,e,d]", "[d,d,e,e] longer e")
R3_HUB_TARGETS = 112


def run_boundaries():
    """one query (118 k-mer starts: the second production tier, the largest miniature tier) whose hits fall into every target of the database:
    the first target (a lone hit on byte 0: the predecessor of the sort's first key), 112 targets with a sequence of R1 each (more survivors
    than one wave sorts), three boundary pairs on neighbouring ids, and the last target.  With 118 k-mer starts the query is beyond the 64 of
    the miniature wide kernel, which hands it to the global path: the run boundaries and the hub meet wide_kernel at its production shape,
    stream_kernel at both, and the global path's rule; the miniature wide_kernel sees the two short chains of R12 only"""
    cs = CaseSet("R3")
    rng = random.Random(8300)
    chain = Chain(segments(rng, 10))
    q = cs.query(chain.seq)
    d, e = 6, -27
    tails = _tails(rng)
    r1 = {label: (runs, expect) for label, runs, expect in R1_SEQUENCES}

    def add(label, runs, expect, skip=0):
        runs = [tuple(r) for r in runs]
        runs[0] = runs[0][:3] + (skip,)
        target, hits = plant(chain, runs, tail=next(tails))
        return cs.case("R3", label, q, cs.target(target), hits, expect)

    add("first target, lone 0", [(0, 1, 0)], ("present", 0), skip=4)
    for k in range(R3_HUB_TARGETS):
        label = R3_HUB[k % len(R3_HUB)]
        runs, expect = r1[label]
        dd = d + k // len(R3_HUB)                                        # other bytes from round to round
        if expect != "absent":
            expect = ("present", {"d": dd, "e": e}[expect[1]])
        add("hub " + label, _sym(runs, dd, e), expect, skip=k % 3)
    # a target that ends on byte b, then a target whose only hit has byte b: the second starts from 0 again and is absent
    add("boundary, left [d,d]", [(d, 2, 0)], ("present", d))
    add("boundary, right lone d", [(d, 1, 0)], "absent", skip=5)
    # ... and a target whose only hit has byte 0 behind one that ends on byte b: present
    add("boundary, left [e,d,d]", [(e, 1, 0), (d, 2, 0)], ("present", d))
    add("boundary, right lone 0", [(0, 1, 0)], ("present", 0), skip=7)
    add("boundary, left [d,e]", [(d, 1, 0), (e, 1, 0)], "absent")
    add("boundary, right lone e", [(e, 1, 0)], "absent", skip=2)
    add("last target, [d,d]", [(d, 2, 0)], ("present", d), skip=8)
    return cs


# ---- S: the scorer's alignments ------------------------------------------------------------------------------------------------------------
S_LENGTHS = tuple(range(11, 20))
S_FILLERS = (13, 14, 15)                    # 1, 2, 3 mod 4 between the four copies of the 80-residue query: its offsets are 0, 1, 3, 2 mod 4
S_NEG_LENGTHS = (11, 14, 17, 19)
S_LONE = (1, 6, 11, 16)


def scorer_shape(q_off, q_len, t_off, t_len, diagonal):
    """(query alignment, target alignment, overlap mod 4) of ungapped_score_dwords (mk_prefilter.hip:1661) for a pair on `diagonal`"""
    if diagonal >= 0:
        q0, t0, n = diagonal, 0, min(t_len, q_len - diagonal)
    else:
        q0, t0, n = 0, -diagonal, min(t_len + diagonal, q_len)
    return (q_off + q0) & 3, (t_off + t0) & 3, n & 3


def scorer_alignment():
    """an 80-residue query at the offsets 0, 1, 3, 2 mod 4; targets that are exactly query[p:p + len] (diagonal +p, len - 9 hits, overlap len) for
    len = 11 .. 19 and p = 0 .. 3 mod 4, and targets random(r) + query[0:len] (diagonal -r), ordered so that the targets' offsets take every
    value mod 4 with every overlap mod 4"""
    cs = CaseSet("S")
    rng = random.Random(8500)
    base = _rand(rng, 80)
    qs = []
    for k in range(4):
        qs.append(cs.query(base))
        if k < 3:
            cs.query(_rand(rng, S_FILLERS[k]))
    todo = []
    for j, n in enumerate(S_LENGTHS):
        for m in range(4):
            p = 4 * ((3 * j + 5 * m) % 15) + m                             # p = m mod 4, spread over the query
            todo.append((p, n, base[p:p + n]))
    for r in range(1, 5):
        for n in S_NEG_LENGTHS:
            todo.append((-r, n, _rand(rng, r) + base[:n]))
    for p in S_LONE:                                                       # one k-mer, one hit off byte 0: never a candidate, never scored
        todo.append((p, SPAN, base[p:p + SPAN]))
    # order: at the running offset take the first target that brings an (alignment, tail) not seen yet
    seen, off = set(), 0
    while todo:
        key = lambda it: ((off + max(0, -it[0])) & 3, it[1] & 3, it[0] < 0)
        k = next((i for i, it in enumerate(todo) if key(it) not in seen), 0)
        seen.add(key(todo[k]))
        diag, n, s = todo.pop(k)
        t = cs.target(s)
        off += len(s)
        for q in qs:
            cs.case("S", "S len %d %s" % (n, "p %d" % diag if diag >= 0 else "r %d" % -diag), q, t, [diag] * (n - 9),
                    ("present", diag) if n > SPAN else "absent")
    return cs


def scorer_coverage(cs, q_off, t_off):
    """the (query alignment, target alignment, tail) triples of the S cases on positive and on negative diagonals, from sequence offsets"""
    pos, neg = set(), set()
    for c in cs.cases:
        if c.expect == "absent":
            continue
        d = c.hits[0]
        shape = scorer_shape(int(q_off[c.q]), int(q_off[c.q + 1] - q_off[c.q]), int(t_off[c.t]), int(t_off[c.t + 1] - t_off[c.t]), d)
        (pos if d >= 0 else neg).add(shape)
    return pos, neg


# ---- T: tier edges -------------------------------------------------------------------------------------------------------------------------
def tier_maxpos():
    prod, mini = tiers()
    return sorted({t[2] for t in prod} | {t[2] for t in mini})


def tier_edges():
    """plain random queries of maxpos + 9 and maxpos + 10 residues (maxpos and maxpos + 1 k-mer starts) for every k-mer-start limit of both tier
    sets, each with a mutated copy of a 40-residue slice in three targets"""
    cs = CaseSet("T")
    rng = random.Random(8700)
    for mp in tier_maxpos():
        for L in (mp + 9, mp + 10):
            base = _rand(rng, L)
            q = cs.query(base)
            for _ in range(3):
                a = rng.randrange(0, L - 40 + 1) if L > 40 else 0
                t = cs.target(_rand(rng, rng.randrange(5, 40)) + _mutate(rng, base[a:a + 40], 0.1) + _rand(rng, rng.randrange(5, 40)))
                cs.case("T", "T maxpos %d, %d residues" % (mp, L), q, t, [], ("present", None))
    for _ in range(12):
        cs.target(_rand(rng, rng.randrange(40, 200)))
    return cs


# ---- TL / TK: tier edges at which the limit is the deciding condition -------------------------------------------------------------------------
# tier_classify_kernel (mk_prefilter.hip:1019-1022) passes a query on from tier t when its similar k-mers exceed limit[t] OR its k-mer starts
# exceed maxpos[t].  limit[t] = cap[t] / (hits per similar k-mer * margin) (:2800-2801): 0.05 hits per similar k-mer until tier t has run on
# the database and max(0.01, what it measured) afterwards (:2905), a margin of 1.15 that moves only after 256 queries (:1962, :2907).  A plain
# random query has about 1 200 similar k-mers per start: at the miniature shapes the queries of T leave the small tiers for their k-mer
# count, whatever their length.  The queries here are built so that the length decides.
HPK_FRESH, HPK_FLOOR, MARGIN = 0.05, 0.01, 1.15
TL_KMERS_MOST = 4000                        # below the smallest limit of either set on an untouched database: 256 / (0.05 * 1.15) = 4452
TK_RESIDUES, TK_FILLERS = 26, 5             # 17 k-mer starts of plain residues: their similar k-mers vary a lot, the seed is chosen for the window


def tier_limits(tier_set, hpk=HPK_FRESH):
    return [cap / (hpk * MARGIN) for cap, _, _, _ in tier_set]


def tier_by_length(tier_set, npos):
    """the tier a query of npos k-mer starts is assigned to when its similar k-mers are below every limit: the first with maxpos >= npos,
    None (the global path) behind the last"""
    return next((t for t, row in enumerate(tier_set) if npos <= row[2]), None)


def tier_edges_by_length():
    """TL: for every k-mer-start limit of both tier sets a query of maxpos + 9 and one of maxpos + 10 residues with ONE k-mer: a segment and X
    behind it (X on a used position: no k-mer).  Its copy at the front of one target is a lone hit on diagonal 0, which the rule keeps.  The
    host test holds every query's similar k-mers under TL_KMERS_MOST, so the number of k-mer starts alone decides the tier"""
    cs = CaseSet("TL")
    rng = random.Random(8902)
    mps = tier_maxpos()
    pool = segments(rng, 2 * len(mps))
    for mp in mps:
        for L in (mp + 9, mp + 10):
            seg = pool.pop(0)
            q = cs.query(seg + "X" * (L - SPAN))
            cs.case("TL", "TL maxpos %d, %d residues" % (mp, L), q, cs.target(seg + "X" * rng.randrange(3, 30)), [0], ("present", 0))
    return cs


def tier_edge_by_kmers():
    """TK: the third miniature tier shares its 64 k-mer starts with the second, so no query reaches it by length; it takes the queries of at most
    64 starts whose similar k-mers are beyond limit[1] and within limit[2].  Two queries of 73 and 74 residues -- plain random residues in
    front, X behind -- whose similar k-mers lie between the two limits of a database the tiers have not run on yet (the host test holds them
    there): the first belongs to the third tier, the second, one k-mer start longer, to the fourth.  Each has a copy of its residues in
    three targets"""
    cs = CaseSet("TK")
    rng = random.Random(8940)
    mp = tiers()[1][2][2]
    heads = [_rand(rng, TK_RESIDUES) for _ in range(2)]
    for L, head in zip((mp + 9, mp + 10), heads):
        q = cs.query(head + "X" * (L - len(head)))
        for _ in range(3):
            t = cs.target(_rand(rng, rng.randrange(5, 40)) + _mutate(rng, head, 0.1) + _rand(rng, rng.randrange(5, 40)))
            cs.case("TK", "TK maxpos %d, %d residues" % (mp, L), q, t, [], ("present", None))
    for _ in range(TK_FILLERS):
        cs.target(_rand(rng, rng.randrange(40, 200)))
    return cs


GROUPS = {"R12": rule_and_byte, "R3": run_boundaries, "S": scorer_alignment, "T": tier_edges, "TL": tier_edges_by_length, "TK": tier_edge_by_kmers}
_BUILT = {}


def group(name):
    """the case set of a group, built once per process"""
    if name not in _BUILT:
        _BUILT[name] = GROUPS[name]()
    return _BUILT[name]
