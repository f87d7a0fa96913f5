"""Hand-made Smith-Waterman cases for the alignment stage (tests/test_sw_cases_host.py, tests/test_gpu_sw_kernels.py): jobs placed at the
tile edges, the 16-step block edges, the prefetch depth, half-filled lane groups and ties of the packed kernels of mk_sw.hip -- as
targets, queries and per-query target lists (what prefilter_result_set takes), every pair with a group label.  Deterministic (seeded).
Every expected value is the oracle's (oracle.sw / oracle.sw_profile); gotoh() is the textbook recurrence the kernels claim to equal.
No GPU and no fixtures here."""
import random
from collections import namedtuple

import oracle

AA = "ACDEFGHIKLMNPQRSTVWY"
TILE_ROWS = (32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024)       # metaeuk_amd/csrc/mk_kernels.hpp: sw_cfg_rows
CELL_LIMIT = 120 * 120                                                 # gotoh() is plain Python: the small pairs only

G1_LENGTHS = (1, 2, 16, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257,
              383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 2049)
G2_QUERIES = (40, 100, 300, 600)                                       # one per lane shape of the score pass
G2_TARGETS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81)
G3_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 64, 65)
G3_LARGE = (2048, 2049)                                                # ORDER_TILE of mk_align.hip and one more
G4_SPACERS = (1, 15, 16, 17, 40)
G4_MOTIFS = (24, 47, 64, 100, 300)
G6_LENGTHS = (33, 129, 385, 769)
SCORE_ROWS_PER_LANE = (2, 3, 4, 6, 8, 12, 16, 12, 16, 24)                # mk_sw.hip: launch_sw_score (sequence queries; 16 lanes up to 256 rows, then 32)
P_COLUMNS = (390, 520, 800)                                            # -> the 512-, 768- and 1024-row tiles
P_FRAGMENTS = (15, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300)      # the classes of swt_kernel end at 64, 128 and 256 rows
P_SIZES = (1, 7, 8, 9)


def tile_cfg(q_len):
    """the tile configuration a query of q_len rows runs on (sw_cfg_of)"""
    c = 0
    while c < len(TILE_ROWS) - 1 and TILE_ROWS[c] < q_len:
        c += 1
    return c


def _rand(rng, n, alphabet=AA):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _mutate(rng, s, rate, indel=0.0):
    out = []
    for ch in s:
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(rng.choice(AA))
        out.append(rng.choice(AA) if rng.random() < rate else ch)
    return "".join(out)


class CaseSet:
    """targets, queries, lists[q] = target numbers (no target twice), labels[q][k] = the group label of pair (q, lists[q][k])"""

    def __init__(self, name, gap_open=11, gap_extend=1, bias=True):
        self.name, self.gap_open, self.gap_extend, self.bias = name, gap_open, gap_extend, bias
        self.targets, self.queries, self.lists, self.labels = [], [], [], []
        self._expected = {}

    @property
    def bias_scale(self):
        return 1.0 if self.bias else 0.0

    def query(self, s):
        self.queries.append(s)
        self.lists.append([])
        self.labels.append([])
        return len(self.queries) - 1

    def target(self, s):
        self.targets.append(s)
        return len(self.targets) - 1

    def pair(self, q, t, label):
        """t: a target number, or a sequence that becomes a new target"""
        if isinstance(t, str):
            t = self.target(t)
        assert t not in self.lists[q]
        self.lists[q].append(t)
        self.labels[q].append(label)
        return t

    def pairs(self):
        for q, l in enumerate(self.lists):
            for k, t in enumerate(l):
                yield q, t, self.labels[q][k]

    def describe(self, q, t):
        k = self.lists[q].index(t)
        return "%s %s: query %d (%d residues) x target %d (%d residues), list of %d" % (
            self.name, self.labels[q][k], q, len(self.queries[q]), t, len(self.targets[t]), len(self.lists[q]))

    def expected(self, lanes=(32, 16)):
        """{(q, t): (score, q_end, t_end, q_start, t_start, rev_mismatch)} from the oracle's striped passes at these SIMD lane counts"""
        if lanes not in self._expected:
            self._expected[lanes] = {(q, t): oracle.sw(self.queries[q], self.targets[t], lanes_byte=lanes[0], lanes_word=lanes[1],
                                                       gap_open=self.gap_open, gap_extend=self.gap_extend, bias_scale=self.bias_scale)
                                     for q, t, _ in self.pairs()}
        return self._expected[lanes]


# ---- the textbook recurrence ------------------------------------------------------------------------------------------------------------
Gotoh = namedtuple("Gotoh", "score first_col min_row rows_at_max cols_at_max")


def gotoh(q, t, gap_open=11, gap_extend=1, bias_scale=1.0):
    """full-matrix affine-gap local alignment, nothing striped: H = max(0, diag + s, E, F), E and F opened from H (gap_open for a gap's first
    residue, gap_extend for every further one), s = int8(sub) + bias8 of the query row.  -> the maximum, the first target column that
    reaches it, the smallest query row with it in that column, how many rows of that column hold it, how many columns reach it"""
    mat = oracle.aln_matrix().astype(int).tolist()
    qc, tc = [int(x) for x in oracle.encode(q)], [int(x) for x in oracle.encode(t)]
    cb = [int(x) for x in oracle.query_bias8(q, bias_scale)]
    n = len(qc)
    H, E = [0] * n, [0] * n                                       # the previous column
    best, first_col, col_rows, cols_at_max = 0, -1, [], 0
    for j, tr in enumerate(tc):
        row = mat[tr]
        Hn = [0] * n
        f, diag, up, colmax = 0, 0, 0, 0
        for i in range(n):
            e = max(E[i] - gap_extend, H[i] - gap_open, 0)        # gap in the query: from the cell on the left
            f = max(f - gap_extend, up - gap_open, 0)             # gap in the target: from the cell above
            h = max(0, diag + row[qc[i]] + cb[i], e, f)
            diag = H[i]
            E[i] = e
            Hn[i] = up = h
            if h > colmax:
                colmax = h
        H = Hn
        if colmax > best:
            best, first_col, cols_at_max = colmax, j, 1
            col_rows = [i for i in range(n) if H[i] == best]
        elif colmax == best and best > 0:
            cols_at_max += 1
    if best == 0:
        return Gotoh(0, -1, -1, 0, 0)
    return Gotoh(best, first_col, col_rows[0], len(col_rows), cols_at_max)


def small(cs, q, t):
    return len(cs.queries[q]) * len(cs.targets[t]) <= CELL_LIMIT


# ---- G1 / G6: tile edges ---------------------------------------------------------------------------------------------------------------
def tile_edges(name="G1", lengths=G1_LENGTHS, **kw):
    """a query of every length around the tile sizes; five targets each: a flanked copy, a copy with indels, a homolog of the last 12 rows only
    (the end cell lies in row L - 1: the last lane, its last register row, beside the padded slots of the 48-row tile), a homolog of the
    first 12 rows only, and a random sequence.  Queries of fewer than 16 rows get a second unmutated copy with other flanks in place of the
    copy with indels (a mutated copy of one or two residues may score nothing), labelled as such"""
    cs = CaseSet(name, **kw)
    for L in lengths:
        rng = random.Random(1000 + L)
        base = _rand(rng, L)
        q = cs.query(base)
        flank = lambda: _rand(rng, rng.randrange(5, 21))
        cs.pair(q, flank() + base + flank(), name + "/copy")
        if L >= 16:
            cs.pair(q, flank() + _mutate(rng, base, 0.1, 0.06) + flank(), name + "/indels")
        else:
            cs.pair(q, flank() + base + flank(), name + "/second copy")
        cs.pair(q, flank() + base[-12:] + flank(), name + "/last rows")
        cs.pair(q, flank() + base[:12] + flank(), name + "/first rows")
        cs.pair(q, (_rand(rng, rng.randrange(40, 100)) if L > 2 else "".join(rng.sample(AA * 2, 40))), name + "/random")
    return cs


def other_gap_costs():
    return tile_edges("G6", G6_LENGTHS, gap_open=7, gap_extend=2)


# ---- G2: column edges ------------------------------------------------------------------------------------------------------------------
def _best_slice(q, k):
    """where the query scores highest against itself over k rows (the short slices must score above 0 on their own)"""
    mat, cb, qc = oracle.aln_matrix(), oracle.query_bias8(q), oracle.encode(q)
    own = [int(mat[c][c]) + int(b) for c, b in zip(qc, cb)]
    return max(range(len(q) - k + 1), key=lambda a: sum(own[a:a + k]))


def column_edges():
    """targets of every length around the 16-step blocks, the G - 1 ramp and the three blocks fetched ahead; for every length one whose
    maximum falls in its LAST column (a slice of the query at its end) and one whose maximum falls in column 0 .. 15 (the query's last rows in
    front).  The two are not the same slice: in front of a random tail only the query's LAST rows cannot be extended by chance into that tail
    (an earlier slice was, and left column 0 .. 15), while the slice at the target's end may lie anywhere in the query.  A third kind, "block
    edge", puts the end cell on the last step of a 16-step block of the score pass"""
    cs = CaseSet("G2")
    for QL in G2_QUERIES:
        rng = random.Random(2000 + QL)
        base = _rand(rng, QL)
        q = cs.query(base)
        lane = (QL - 1) // SCORE_ROWS_PER_LANE[tile_cfg(QL)]        # the lane of the query's last row in the score pass
        for n in G2_TARGETS:
            k = min(n, 14)
            a = _best_slice(base, k) if k < 8 else rng.randrange(0, QL - k + 1)
            cs.pair(q, _rand(rng, n - k) + base[a:a + k], "G2/last column")
            k = min(n, 16)                                          # (the query's last rows: no chance extension into the random tail)
            cs.pair(q, base[QL - k:] + _rand(rng, n - k), "G2/early column")
            # ... and one whose end cell is computed in the LAST step of a block of 16 of the score pass ((column + lane) % 16 == 15) and not in
            # the target's last column: the column bound that pass hands to the position pass (min(cA, lastA)) is then exact, nothing to spare
            ends = [e for e in range(k - 1, n - 1) if (e + lane) % 16 == 15]
            if ends and k == 16:
                cs.pair(q, _rand(rng, ends[-1] - k + 1) + base[QL - k:] + _rand(rng, n - ends[-1] - 1), "G2/block edge")
    return cs


# ---- G3: wave shapes -------------------------------------------------------------------------------------------------------------------
def wave_shapes():
    """lists of every size around the jobs per wave (8, 4, 1), ORDER_WAVE_MAX = 64 and ORDER_TILE = 2048 of the planner, and three lists of two
    targets of very different lengths.  The pairs on tiles of at most 64 rows are no multiple of 8: the last wave of the packed position
    kernel is half filled"""
    cs = CaseSet("G3")
    rng = random.Random(3000)
    for QL, lo, hi in ((60, 25, 60), (400, 40, 200)):
        base = _rand(rng, QL)
        pool = []
        for k in range(max(G3_SIZES)):
            if k % 2 == 0:
                n = rng.randrange(lo, hi + 1)
                a = rng.randrange(0, QL - n + 1)
                pool.append(cs.target(_rand(rng, rng.randrange(0, 21)) + _mutate(rng, base[a:a + n], 0.15) + _rand(rng, rng.randrange(0, 21))))
            else:
                pool.append(cs.target(_rand(rng, rng.randrange(30, 121))))
        for size in G3_SIZES:
            q = cs.query(base)
            for t in rng.sample(pool, size):
                cs.pair(q, t, "G3/list of %d" % size)
        if QL == 60:
            q60 = base
    qa, qb = _rand(rng, 40), _rand(rng, 40)
    pool = []
    for k in range(max(G3_LARGE)):
        n = rng.randrange(20, 41)
        if k % 2 == 0:
            src = qa if k % 4 == 0 else qb
            a = rng.randrange(0, 40 - n + 1)
            pool.append(cs.target(_mutate(rng, src[a:a + n], 0.2)))
        else:
            pool.append(cs.target(_rand(rng, n)))
    for base, size in zip((qa, qb), G3_LARGE):
        q = cs.query(base)
        for t in rng.sample(pool, size):
            cs.pair(q, t, "G3/list of %d" % size)
    a = _best_slice(q60, 1)
    for name, two in (("lengths 1 and 300", (q60[a], _rand(rng, 300))),
                      ("lengths 16 and 17", (q60[5:21], q60[30:47])),
                      ("random 300 and homolog 20", (_rand(rng, 300), q60[22:42]))):
        q = cs.query(q60)
        for s in two:
            cs.pair(q, s, "G3/two targets, " + name)
    return cs


# ---- G4: ties and repeated maxima (composition bias off: with it the rows of a repeated motif differ and the ties vanish) ------------------
def stripe_adversaries():
    """the pairs of tests/test_gpu_parity.py::test_sw_stripe_semantics (same seed, same draws): a query gap next to a target gap"""
    rng = random.Random(3)
    out = []
    for rep in range(60):
        a, b, c = _rand(rng, rng.randrange(20, 60)), _rand(rng, rng.randrange(8, 30)), _rand(rng, rng.randrange(20, 60))
        ins = _rand(rng, rng.randrange(8, 30))
        out.append((a + b + c, a + ins + c))
        out.append((a + c, a + ins + c))
    return out


def ties():
    cs = CaseSet("G4", bias=False)
    rng = random.Random(4000)
    for M in G4_MOTIFS:
        m = _rand(rng, M)
        qa, qb = cs.query(m), cs.query(m)
        for sp in G4_SPACERS:
            spacer = _rand(rng, sp)
            # (a) the same maximum at the end of both copies: the first column wins
            cs.pair(qa, m + spacer + m, "G4/a twice, spacer %d" % sp)
            # (b) one substitution in the first copy: the maximum rises in the second
            at = M // 2
            worse = m[:at] + ("P" if m[at] != "P" else "G") + m[at + 1:]
            cs.pair(qb, worse + spacer + m, "G4/b second copy, spacer %d" % sp)
            # (c) the motif twice in the QUERY: one column, two rows (two lanes) -- the smallest row wins
            cs.pair(cs.query(m + spacer + m), m, "G4/c two rows, spacer %d" % sp)
    # (d) a tie inside one lane's rows: WWC at rows 0 and 8 of a 160-residue query without another W, C or P (12 rows per lane), ...
    plain = "ADEGHIKLMNQRSTV"                                      # (no F / Y either: they score above 0 against W)
    body = _rand(rng, 160, plain)
    cs.pair(cs.query("WWC" + body[3:8] + "WWC" + body[11:]), "PPPPPWWCPPPPPP", "G4/d one lane, WWC twice")
    # ... and in the tiles of the packed position kernel (2, 3 and 4 rows per lane): WW at rows 4 and 5 against a single W
    for L in (30, 45, 60):
        body = _rand(rng, L, plain)
        cs.pair(cs.query(body[:4] + "WW" + body[6:]), "PPPWPPP", "G4/d one lane, WW")
    # (e)
    for qs, ts in stripe_adversaries():
        cs.pair(cs.query(qs), ts, "G4/e stripe adversary")
    return cs


# ---- G5: nothing to find ---------------------------------------------------------------------------------------------------------------
def nothing_to_find():
    """score 0 (no record), scores of 1 .. 3, one-residue targets"""
    cs = CaseSet("G5")
    rng = random.Random(5000)
    ps = [cs.target("P" * n) for n in (1, 17, 40)]
    ws = [cs.target("W" * n) for n in (1, 2, 30)]
    for n in (20, 48, 100, 300, 600, 1100):
        q = cs.query("W" * n)
        for t in ps:
            cs.pair(q, t, "G5/poly-W x poly-P")
        for t in ws:
            cs.pair(q, t, "G5/poly-W x poly-W")                     # (the query's own composition bias takes W x W down to nothing)
    found = 0
    for _ in range(2000):                                           # seeded search for the smallest positive scores, decided by the oracle
        qs, ts = _rand(rng, rng.randrange(30, 70)), _rand(rng, rng.randrange(1, 3))
        if 1 <= oracle.sw(qs, ts, with_start=False)[0] <= 3:
            cs.pair(cs.query(qs), ts, "G5/low score")
            found += 1
            if found == 6:
                break
    base = _rand(rng, 50)
    q = cs.query(base)
    cs.pair(q, base[_best_slice(base, 1)], "G5/one-residue target")
    cs.pair(q, "P" if "P" not in base else "W", "G5/one-residue target")
    return cs


SEQUENCE_GROUPS = {"G1": tile_edges, "G2": column_edges, "G3": wave_shapes, "G4": ties, "G5": nothing_to_find, "G6": other_gap_costs}
LANES = {"G4": ((32, 16), (16, 8))}                                  # the groups that run at more than the default SIMD lane counts
_BUILT = {}


def group(name):
    """the case set of a group, built once per process"""
    if name not in _BUILT:
        _BUILT[name] = SEQUENCE_GROUPS[name]()
    return _BUILT[name]


def lanes_of(name):
    return LANES.get(name, ((32, 16),))


# ---- P: profile queries ----------------------------------------------------------------------------------------------------------------
def synthetic_profile(rng, length, favoured=(12, 40)):
    """a profile DB entry (25 bytes per column) with random integer scores, as tests/test_gpu_profile.py::_synthetic_profile -> (entry, consensus)"""
    out = bytearray()
    for _ in range(length):
        fav = rng.randrange(20)
        col = [rng.randint(-24, 6) for _ in range(20)]
        col[fav] = rng.randint(*favoured)
        for _ in range(rng.randrange(3)):
            col[rng.randrange(20)] = rng.randint(0, 20)
        out += bytes((v & 0xFF) for v in col) + bytes([fav, fav, 10, 0, 0])
    return bytes(out) + b"\0", "".join(AA[max(range(20), key=lambda a: ((out[25 * i + a] + 128) % 256))] for i in range(length))


class ProfileSet:
    def __init__(self):
        self.name = "P"
        self.entries, self.columns, self.targets, self.lists, self.labels = [], [], [], [], []
        self._expected = None

    def pairs(self):
        for q, l in enumerate(self.lists):
            for k, t in enumerate(l):
                yield q, t, self.labels[q][k]

    def describe(self, q, t):
        k = self.lists[q].index(t)
        return "P %s: profile %d (%d columns) x fragment %d (%d residues), list of %d" % (
            self.labels[q][k], q, self.columns[q], t, len(self.targets[t]), len(self.lists[q]))

    def expected(self, lanes=(32, 16)):
        if self._expected is None:
            self._expected = {}
            for q, l in enumerate(self.lists):
                res = oracle.sw_profile(self.entries[q], self.columns[q], [self.targets[t] for t in l], lanes_byte=lanes[0], lanes_word=lanes[1])
                for t, r in zip(l, res):
                    self._expected[(q, t)] = r
        return self._expected


def profiles():
    """profiles of 390, 520 and 800 columns (the 512-, 768- and 1024-row tiles) against fragments of their consensus whose lengths straddle the
    classes of the transposed kernels (64, 128, 256 rows) and their 256-row limit; lists of 1, 7, 8 and 9; waves that mix a 257-residue
    fragment with short ones (the whole wave takes the classic kernel); a profile with favoured scores of ~120 (30 per row in the alignment
    profile) whose 300-residue fragment scores far beyond what the byte pass holds"""
    ps = ProfileSet()
    rng = random.Random(6000)

    def add_query(entry, n_cols, frag_ids, label):
        ps.entries.append(entry)
        ps.columns.append(n_cols)
        ps.lists.append(list(frag_ids))
        ps.labels.append([label] * len(frag_ids))

    for n_cols, favoured in [(c, (12, 40)) for c in P_COLUMNS] + [(520, (116, 124))]:
        entry, cons = synthetic_profile(rng, n_cols, favoured)
        frag = {}
        for n in P_FRAGMENTS:
            for v in range(3):
                a = rng.randrange(0, n_cols - n + 1)
                s = "".join(rng.choice(AA) if rng.random() < 0.15 else ch for ch in cons[a:a + n])
                ps.targets.append(s)
                frag[(n, v)] = len(ps.targets) - 1
        hot = favoured[0] > 100
        tag = "hot %d" % n_cols if hot else "%d columns" % n_cols
        if hot:
            a = rng.randrange(0, n_cols - 300 + 1)
            ps.targets.append(cons[a:a + 300])                         # the unmutated consensus fragment
            add_query(entry, n_cols, [len(ps.targets) - 1], tag + "/consensus 300")
        add_query(entry, n_cols, [frag[(300, 0)]], tag + "/list of 1, 300 residues")
        add_query(entry, n_cols, [frag[(257, 0)]], tag + "/list of 1, 257 residues")
        add_query(entry, n_cols, [frag[(15, 0)]], tag + "/list of 1, 15 residues")
        add_query(entry, n_cols, [frag[(n, 0)] for n in (15, 63, 64, 65, 127, 128, 129)], tag + "/list of 7, up to 129")
        add_query(entry, n_cols, [frag[(15, v)] for v in range(3)] + [frag[(63, v)] for v in range(2)] + [frag[(64, v)] for v in range(2)],
                  tag + "/list of 7, up to 64")
        add_query(entry, n_cols, [frag[(n, 1)] for n in (15, 63, 64, 65, 127, 128, 255, 256)], tag + "/list of 8, up to 256")
        add_query(entry, n_cols, [frag[(n, 2)] for n in (65, 127, 128)] + [frag[(n, 1)] for n in (65, 127, 128)] + [frag[(129, 1)], frag[(129, 2)]],
                  tag + "/list of 8, 65 .. 129")
        add_query(entry, n_cols, [frag[(257, 1)]] + [frag[(n, 2)] for n in (15, 63, 64)] +[frag[(n, 0)] for n in (63, 64, 65, 127)],
                  tag + "/list of 8, 257 among short ones")
        add_query(entry, n_cols, [frag[(n, 2)] for n in (257, 15, 63, 64, 255, 256, 300)] + [frag[(129, 0)], frag[(255, 0)]],
                  tag + "/list of 9, 257 and 300 among the others")
    return ps


def profile_group():
    if "P" not in _BUILT:
        _BUILT["P"] = profiles()
    return _BUILT["P"]
