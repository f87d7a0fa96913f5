#!/bin/bash
# Process-level goldens of --max-accept / --max-rejected (Alignment.cpp:343-405) from the REAL reference binary, made like the backtrace and the
# ORF-flag ones (make_backtrace_golden.sh): the binary is built OUTSIDE the repository from a copy of the read-only reference tree; nothing of
# it is kept, only its OUTPUT DBs become fixtures (data), as '>key' blocks sorted by key.
# `align aa_6f targetsDB pref_0 ... --alignment-mode 2 --min-aln-len 11` on the real process's prefilter DB (checked to equal e2e_process_pref):
#   e2e_limit_aln_A.txt.gz            -e 100 --max-accept 1
#   e2e_limit_aln_B.txt.gz            -e 100 --max-rejected 1
#   e2e_limit_aln_C.txt.gz            -e 0.001 --max-accept 1 --max-rejected 2      (e2e_limit_aln_C_unlimited.txt.gz: the same -e without limits)
#   e2e_limit_aln_D.txt.gz            -e 100 -c 0.2 --cov-mode 5 --max-rejected 1   (e2e_limit_aln_D_unlimited.txt.gz: without the limit).  The pairs that fail
#                                     the length test stay in this list and end streaks; of the settings tried (-c 0.15 to 0.5, modes 0, 1, 5) this one
#                                     has the most queries whose result depends on such a rejection
# `predictexons contigsDB targetsDB ... -s 5.7`:
#   e2e_limit_search_res_acc1.txt.gz / e2e_limit_calls_acc1.txt.gz      --max-accept 1
#   e2e_limit_search_res_m3a.txt.gz / e2e_limit_calls_m3a.txt.gz        --alignment-mode 3 -a 1 --max-accept 2 --max-rejected 2 -e 0.001
# No case may pass on nothing: the script walks the recorded lists with the rule itself (accepted set = the unlimited output of the same settings),
# checks that the walk reproduces every limited output, and asserts the counts below; they are recorded in PROVENANCE_align_limits.txt.
# Inputs: tests/golden/e2e_targets.txt.gz, e2e_contigs.txt.gz (createdb --shuffle 0, so keys = line numbers).  Host L2 = 2097152.
# An existing binary is used when METAEUK names one (or make_process_golden.sh left its build behind).
set -e
R=$(cd $(dirname $0)/../.. && pwd)
W=${1:-$(mktemp -d /tmp/alg.XXXXXX)}
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
import gzip
def lines(n): return gzip.open('$R/tests/golden/' + n, 'rt').read().splitlines()
open('targets.faa', 'w').write("".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_targets.txt.gz'))))
open('contigs.fna', 'w').write("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_contigs.txt.gz'))))
PY
$M createdb targets.faa targetsDB --shuffle 0 > /dev/null
$M createdb contigs.fna contigsDB --shuffle 0 > /dev/null
mkdir tmp tmp1 tmp2 tmp3
$M predictexons contigsDB targetsDB calls tmp --remove-tmp-files 0 --threads 4 -s 5.7 > run.log 2>&1
$M predictexons contigsDB targetsDB calls1 tmp1 --remove-tmp-files 0 --threads 4 -s 5.7 --max-accept 1 > run1.log 2>&1
$M predictexons contigsDB targetsDB calls2 tmp2 --remove-tmp-files 0 --threads 4 -s 5.7 --alignment-mode 3 -a 1 --max-accept 2 --max-rejected 2 -e 0.001 > run2.log 2>&1
$M predictexons contigsDB targetsDB calls3 tmp3 --remove-tmp-files 0 --threads 4 -s 5.7 --alignment-mode 3 -a 1 -e 0.001 > run3.log 2>&1
Q=tmp/latest/aa_6f
P=$(ls tmp/latest/tmp_search/*/pref_0.index | head -1); P=${P%.index}
A="--alignment-mode 2 --min-aln-len 11 --threads 4"
$M align $Q targetsDB $P alnA $A -e 100 --max-accept 1 > alnA.log 2>&1
$M align $Q targetsDB $P alnB $A -e 100 --max-rejected 1 > alnB.log 2>&1
$M align $Q targetsDB $P alnC $A -e 0.001 --max-accept 1 --max-rejected 2 > alnC.log 2>&1
$M align $Q targetsDB $P alnC0 $A -e 0.001 > alnC0.log 2>&1
$M align $Q targetsDB $P alnD $A -e 100 -c 0.2 --cov-mode 5 --max-rejected 1 > alnD.log 2>&1
$M align $Q targetsDB $P alnD0 $A -e 100 -c 0.2 --cov-mode 5 > alnD0.log 2>&1
python3 - <<PY
import glob, gzip, os
import numpy as np
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
def gold(n): return gzip.open(G + n, 'rt').read()
def parse(text):
    out, k = {}, None
    for l in text.splitlines():
        if l.startswith('>'): k = int(l[1:]); out[k] = []
        elif l: out[k].append(l)
    return out
pref = read_db('$P')
assert blocks(pref) == gold('e2e_process_pref.txt.gz'), "this run's prefilter DB differs from the committed e2e_process_pref"
assert blocks(read_db('$W/tmp/latest/search_res')) == gold('e2e_process_aln.txt.gz'), "this run's default search_res differs from e2e_process_aln"
lists = {k: [int(l.split('\t')[0]) for l in v] for k, v in parse(blocks(pref)).items()}
qlen = {k: len(v) - 1 for k, v in read_db('$W/$Q').items()}
tlen = {k: len(v) - 1 for k, v in read_db('$W/targetsDB').items()}
def covered(q, t, thr=np.float32(0.2)):               # Util::canBeCovered, --cov-mode 5, float arithmetic
    a, b = np.float32(qlen[q]), np.float32(tlen[t])
    return min(a, b) / max(a, b) >= thr
def walk(unlimited, max_acc, max_rej, cut=False, drop_cut=False):
    """the rule on the recorded lists -> (kept blocks, stops by accept, stops by rejection, pairs looked at)"""
    kept, sa, sr, looked = {}, 0, 0, 0
    for q, lst in lists.items():
        acc = {int(l.split('\t')[0]): l for l in unlimited.get(q, [])}
        passed = streak = 0
        keep = []
        for t in lst:
            if not (passed < max_acc and streak < max_rej): break
            if cut and not covered(q, t):
                if drop_cut: continue
                looked += 1; streak += 1; continue
            looked += 1
            if t in acc: keep.append(acc[t]); passed += 1; streak = 0
            else: streak += 1
        sa += passed >= max_acc; sr += streak >= max_rej and passed < max_acc
        kept[q] = keep
    return kept, sa, sr, looked
def same_sets(kept, limited):                       # (the limited output is sorted; the order is checked by the tests against the library)
    return all(sorted(kept.get(q, [])) == sorted(limited.get(q, [])) for q in lists)
INF = 2 ** 31 - 1
report = ["pairs in the recorded lists: %d, fragments: %d" % (sum(len(v) for v in lists.values()), len(lists))]
def case(name, db, unl_text, max_acc, max_rej, cut=False):
    lim_text = blocks(read_db(db))
    assert lim_text != unl_text, "case %s equals the unlimited output" % name
    unl, lim = parse(unl_text), parse(lim_text)
    kept, sa, sr, looked = walk(unl, max_acc, max_rej, cut)
    assert same_sets(kept, lim), "case %s: the rule on the recorded lists does not reproduce the reference's output" % name
    changed = sum(1 for q in lists if unl.get(q, []) != lim.get(q, []))
    report.append("case %s: %d stops by accept, %d stops by rejection, %d results changed, %d pairs looked at" % (name, sa, sr, changed, looked))
    return lim_text, sa, sr, changed, kept
t, sa, sr, ch, _ = case('A', '$W/alnA', gold('e2e_process_aln.txt.gz'), 1, INF); assert sa >= 400; write('e2e_limit_aln_A.txt.gz', t)
t, sa, sr, ch, _ = case('B', '$W/alnB', gold('e2e_process_aln.txt.gz'), INF, 1); assert sr >= 50 and ch >= 20; write('e2e_limit_aln_B.txt.gz', t)
c0 = blocks(read_db('$W/alnC0')); write('e2e_limit_aln_C_unlimited.txt.gz', c0)
t, sa, sr, ch, _ = case('C', '$W/alnC', c0, 1, 2); assert sa >= 50 and sr >= 50; write('e2e_limit_aln_C.txt.gz', t)
d0 = blocks(read_db('$W/alnD0')); write('e2e_limit_aln_D_unlimited.txt.gz', d0)
t, sa, sr, ch, keptD = case('D', '$W/alnD', d0, INF, 1, cut=True); write('e2e_limit_aln_D.txt.gz', t)
blind, _, _, _ = walk(parse(d0), INF, 1, cut=True, drop_cut=True)      # the walk without the length-test rejections
dep = sum(1 for q in lists if sorted(blind[q]) != sorted(keptD[q]))
report.append("case D: %d queries whose result depends on a length-test rejection" % dep)
assert dep >= 5
s1, c1 = blocks(read_db('$W/tmp1/latest/search_res')), blocks(read_db('$W/calls1'))
assert s1 != gold('e2e_process_aln.txt.gz') and s1 == gold('e2e_limit_aln_A.txt.gz'), "predictexons --max-accept 1: search_res should equal case A"
write('e2e_limit_search_res_acc1.txt.gz', s1); write('e2e_limit_calls_acc1.txt.gz', c1)
report.append("predictexons --max-accept 1: search_res == case A; dp_predictions %s the default's" % ("differ from" if c1 != gold('e2e_exons_expected.txt.gz') else "EQUAL"))
s2, c2, s3 = blocks(read_db('$W/tmp2/latest/search_res')), blocks(read_db('$W/calls2')), blocks(read_db('$W/tmp3/latest/search_res'))
assert s2 != s3, "the mode-3 case equals its unlimited run"
n2, n3 = sum(len(v) for v in parse(s2).values()), sum(len(v) for v in parse(s3).values())
report.append("predictexons --alignment-mode 3 -a 1 -e 0.001: %d records without limits, %d with --max-accept 2 --max-rejected 2" % (n3, n2))
write('e2e_limit_search_res_m3a.txt.gz', s2); write('e2e_limit_calls_m3a.txt.gz', c2)
print("\n".join(report))
PY
