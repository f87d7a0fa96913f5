#!/bin/bash
# Process-level goldens of --alignment-mode 3 / -a (the banded backtrace, exact identities) from the REAL reference binary, made like the filter
# ones (make_filter_golden.sh): the binary is built OUTSIDE the repository from a copy of the read-only reference tree; nothing of it is kept,
# only its OUTPUT DBs become fixtures (data), as '>key' blocks sorted by key:
#   e2e_process_aln_m3a.txt.gz / e2e_process_calls_m3a.txt.gz              search_res (11 columns) and dp_predictions of
#                                                                         `predictexons ... -s 5.7 --alignment-mode 3 -a 1` on the e2e fixture
#   e2e_process_aln_m3a_id03.txt.gz / e2e_process_calls_m3a_id03.txt.gz   ... the same with --min-seq-id 0.3 --seq-id-mode 1
#   bt_corner_{queries,targets,classes,aln}.txt.gz                        createdb + prefilter + `align -a 1 --alignment-mode 3 -e 100` on hand-made
#                                                                         pairs (query i belongs to target i; the prefilter adds what else it finds):
#     a  no indel            b  3-residue insertion, 30 identical residues, 3-residue deletion (square rectangle: the band goes 1, 2, 4)
#     c  the same with 40-residue indels (band up to 64)        d  a to c over two- and three-letter alphabets (E / F / H ties)
#     e  one query of 600+ residues against a target half again as long, scattered indels
# Inputs of the e2e runs: tests/golden/e2e_targets.txt.gz, e2e_contigs.txt.gz (createdb --shuffle 0, so keys = line numbers).  Host L2 = 2097152.
# Prints, per class, how many output records carry an I or a D; recorded in PROVENANCE_backtrace.txt.
# An existing binary is used when METAEUK names one (or make_process_golden.sh left its build behind).
set -e
R=$(cd $(dirname $0)/../.. && pwd)
W=${1:-$(mktemp -d /tmp/btg.XXXXXX)}
M=${METAEUK:-/tmp/ref-build/src/metaeuk}
if [ ! -x "$M" ]; then
    mkdir -p /tmp/ref-build
    [ -d /tmp/ref-src ] || cp -r /root/reference /tmp/ref-src
    printf 'stub\nstub\nstub\n' > /tmp/ref-src/lib/mmseqs/data/resources/K4000.crf
    (cd /tmp/ref-build && cmake -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=Release -DHAVE_AVX2=1 /tmp/ref-src > cmake.log && make -j${JOBS:-7} metaeuk > make.log)
    M=/tmp/ref-build/src/metaeuk
fi
mkdir -p $W && cd $W
python3 - <<PY
import gzip, random
G = '$R/tests/golden/'
def lines(n): return gzip.open(G + n, 'rt').read().splitlines()
open('targets.faa', 'w').write("".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_targets.txt.gz'))))
open('contigs.fna', 'w').write("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_contigs.txt.gz'))))
# ---- the corner pairs
rng = random.Random(20261021)
AA = "ACDEFGHIKLMNPQRSTVWY"
def rs(n, alpha=AA): return "".join(rng.choice(alpha) for _ in range(n))
def mut(s, r, alpha=AA): return "".join(c if rng.random() > r else rng.choice(alpha) for c in s)
def pair_a(alpha):
    f = rs(rng.randrange(60, 151), alpha)
    return f, mut(f, 0.1, alpha)
def pair_shift(alpha, k, mid):     # query = A X B C, target = A B Y C: k-residue insertion, |B| identical residues, k-residue deletion
    n = rng.randrange(max(60, 3 * mid), 151) if 3 * mid <= 150 else 3 * mid
    a = (n - mid) // 2
    f = rs(n, alpha)
    A, B, C = f[:a], f[a:a + mid], f[a + mid:]
    return A + rs(k, alpha) + B + C, A + B + rs(k, alpha) + C
def pair_e():
    f = rs(rng.randrange(620, 700))
    q, t = [], []
    for c in f:
        x = rng.random()
        if x < 0.012: q.append(rs(rng.randrange(1, 6)))            # residues only the query has
        elif x < 0.024: t.append(rs(rng.randrange(1, 6)))          # residues only the target has
        q.append(c); t.append(c if rng.random() > 0.08 else rng.choice(AA))
    q, t = "".join(q), "".join(t)
    pad = max(len(q) * 3 // 2 - len(t), 20)
    return q, rs(pad // 2) + t + rs(pad - pad // 2)
Q, T, K = [], [], []
def add(cls, p): Q.append(p[0]); T.append(p[1]); K.append(cls)
for _ in range(60): add('a', pair_a(AA))
for _ in range(60): add('b', pair_shift(AA, 3, 30))
for _ in range(60): add('c', pair_shift(AA, 40, rng.randrange(30, 41)))
for alpha in ("AG", "LKE"):
    for _ in range(15): add('d', pair_a(alpha))
    for _ in range(15): add('d', pair_shift(alpha, 3, 30))
    for _ in range(15): add('d', pair_shift(alpha, 40, rng.randrange(30, 41)))
for alpha in ("AW", "CHW"):      # (high-scoring letters: the scores survive the composition bias correction)
    for _ in range(10): add('d', pair_shift(alpha, 3, 30))
    for _ in range(10): add('d', pair_shift(alpha, 40, rng.randrange(30, 41)))
for _ in range(3): add('e', pair_e())
def write(n, t):
    with gzip.open(G + n, 'wt', compresslevel=9) as f: f.write(t)
write('bt_corner_queries.txt.gz', "\n".join(Q) + "\n")
write('bt_corner_targets.txt.gz', "\n".join(T) + "\n")
write('bt_corner_classes.txt.gz', "\n".join(K) + "\n")
open('cq.faa', 'w').write("".join(">q%d\n%s\n" % (i, s) for i, s in enumerate(Q)))
open('ct.faa', 'w').write("".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(T)))
PY
$M createdb targets.faa targetsDB --shuffle 0 > /dev/null
$M createdb contigs.fna contigsDB --shuffle 0 > /dev/null
$M createdb cq.faa cqDB --shuffle 0 > /dev/null
$M createdb ct.faa ctDB --shuffle 0 > /dev/null
mkdir tmp tmp2
$M predictexons contigsDB targetsDB calls tmp --remove-tmp-files 0 --threads 4 -s 5.7 --alignment-mode 3 -a 1 > run.log 2>&1
$M predictexons contigsDB targetsDB calls2 tmp2 --remove-tmp-files 0 --threads 4 -s 5.7 --alignment-mode 3 -a 1 --min-seq-id 0.3 --seq-id-mode 1 > run2.log 2>&1
$M prefilter cqDB ctDB cpref -s 7.5 --mask 0 --threads 4 > cpref.log 2>&1
$M align cqDB ctDB cpref caln -a 1 --alignment-mode 3 -e 100 --threads 4 > caln.log 2>&1
python3 - <<PY
import glob, gzip, os, re
def read_db(base):
    if os.path.exists(base): data = open(base, 'rb').read()
    else:
        data, i = b'', 0
        while os.path.exists(base + '.%d' % i): data += open(base + '.%d' % i, 'rb').read(); i += 1
    return {int(l.split('\t')[0]): data[int(l.split('\t')[1]):int(l.split('\t')[1]) + int(l.split('\t')[2]) - 1].decode() for l in open(base + '.index')}
G = '$R/tests/golden/'
blocks = lambda d: "".join(">%d\n%s" % (k, d[k]) for k in sorted(d))
def write(n, t):
    with gzip.open(G + n, 'wt', compresslevel=9) as f: f.write(t)
write("e2e_process_aln_m3a.txt.gz", blocks(read_db('$W/tmp/latest/search_res')))
write("e2e_process_calls_m3a.txt.gz", blocks(read_db('$W/calls')))
write("e2e_process_aln_m3a_id03.txt.gz", blocks(read_db('$W/tmp2/latest/search_res')))
write("e2e_process_calls_m3a_id03.txt.gz", blocks(read_db('$W/calls2')))
aln = read_db('$W/caln')
write("bt_corner_aln.txt.gz", blocks(aln))
cls = gzip.open(G + 'bt_corner_classes.txt.gz', 'rt').read().split()
own, gapped, band = {}, {}, {}
for k, body in aln.items():
    for l in body.splitlines():
        c = l.split('\t')
        if int(c[0]) != k: continue          # only the pair the class was made for
        own[cls[k]] = own.get(cls[k], 0) + 1
        if 'I' in c[10] or 'D' in c[10]: gapped[cls[k]] = gapped.get(cls[k], 0) + 1
total = sum(len(b.splitlines()) for b in aln.values())
print("corner fixture: %d pairs, %d records in all" % (len(cls), total))
for k in sorted(set(cls)):
    print("class %s: %d pairs, %d own records, %d with an I or a D" % (k, cls.count(k), own.get(k, 0), gapped.get(k, 0)))
e2e = [l for l in gzip.open(G + 'e2e_process_aln_m3a.txt.gz', 'rt').read().splitlines() if not l.startswith('>')]
print("e2e -a: %d records, %d with an I or a D" % (len(e2e), sum(1 for l in e2e if 'I' in l.split('\t')[10] or 'D' in l.split('\t')[10])))
PY
