#!/bin/bash
# Goldens of the ungapped rescoring stage from the REAL reference binary: `metaeuk rescorediagonal aa_6f targetsDB pref_0 out --rescore-mode 2`
# over the prefilter result of the e2e fixture (the pref_0 of `predictexons -s 5.7`, which must equal e2e_process_pref.txt.gz), three ways:
#   e2e_process_rescore.txt.gz          default flags
#   e2e_process_rescore_a_sorted.txt.gz -a 1 --sort-results 1
#   e2e_process_rescore_c05_id03.txt.gz -c 0.5 --cov-mode 2 --min-seq-id 0.3 --seq-id-mode 1 -e 0.001
# Provenance: with the module's defaults (-e 0.001) 2 831 of the 4 777 pairs are kept.  E-values and bit scores are those of the GAPLESS statistics
# (EvalueComputation.h:70-75: rescorediagonal.cpp:107 builds its EvalueComputation without gap costs), not the 11 / 1 set of `align`.
# tests/test_rescore_host.py holds mk_rescore_diagonal_host to the three files, tests/test_gpu_rescore.py the kernel, the command
# `metaeuk-amd rescorediagonal` and `search --alignment-mode 4`.  (tests/golden/PROVENANCE.txt is not extended: this header is the record.)
# The binary is built OUTSIDE the repository from a copy of the reference tree (cmake + make, as make_process_golden.sh does); nothing of it
# is kept, only the three output DBs become fixtures (data), as '>key' blocks sorted by key.
# Usage: make_rescore_golden.sh <reference tree> [work dir] [built metaeuk binary]
set -e
R=$(cd $(dirname $0)/../.. && pwd)
REF=${1:?reference tree}
W=${2:-/tmp/rg}
M=$3
rm -rf $W && mkdir -p $W
if [ -z "$M" ]; then
    rm -rf $W-src $W-build && mkdir -p $W-build
    cp -r $REF $W-src
    printf 'stub\nstub\nstub\n' > $W-src/lib/mmseqs/data/resources/K4000.crf
    (cd $W-build && cmake -DCMAKE_POLICY_VERSION_MINIMUM=3.5 -DCMAKE_BUILD_TYPE=Release -DHAVE_AVX2=1 $W-src > cmake.log && make -j7 metaeuk > make.log)
    M=$W-build/src/metaeuk
fi
cd $W
python3 - <<PY
import gzip
def lines(n): return gzip.open('$R/tests/golden/' + n, 'rt').read().splitlines()
open('targets.faa', 'w').write("".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_targets.txt.gz'))))
open('contigs.fna', 'w').write("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_contigs.txt.gz'))))
PY
$M createdb targets.faa targetsDB --shuffle 0 > /dev/null
$M createdb contigs.fna contigsDB --shuffle 0 > /dev/null
mkdir tmp
$M predictexons contigsDB targetsDB calls tmp --remove-tmp-files 0 --threads 4 -s 5.7 > run.log 2>&1
Q=tmp/latest/aa_6f
P=$(ls tmp/latest/tmp_search/*/pref_0.index | head -1); P=${P%.index}
$M rescorediagonal $Q targetsDB $P resc_default --rescore-mode 2 --threads 4 > r1.log 2>&1
$M rescorediagonal $Q targetsDB $P resc_a_sorted --rescore-mode 2 -a 1 --sort-results 1 --threads 4 > r2.log 2>&1
$M rescorediagonal $Q targetsDB $P resc_c05_id03 --rescore-mode 2 -c 0.5 --cov-mode 2 --min-seq-id 0.3 --seq-id-mode 1 -e 0.001 --threads 4 > r3.log 2>&1
python3 - <<PY
import gzip, os
def read_db(base):
    if os.path.exists(base): data = open(base, 'rb').read()
    else:
        data, i = b'', 0
        while os.path.exists(base + '.%d' % i): data += open(base + '.%d' % i, 'rb').read(); i += 1
    return {int(l.split('\t')[0]): data[int(l.split('\t')[1]):int(l.split('\t')[1]) + int(l.split('\t')[2]) - 1].decode() for l in open(base + '.index')}
G = '$R/tests/golden/'
blocks = lambda d: "".join(">%d\n%s" % (k, d[k]) for k in sorted(d))
assert blocks(read_db('$W/$P')) == gzip.open(G + 'e2e_process_pref.txt.gz', 'rt').read(), "this run's pref_0 differs from e2e_process_pref.txt.gz"
for src, name in (('resc_default', 'e2e_process_rescore'), ('resc_a_sorted', 'e2e_process_rescore_a_sorted'), ('resc_c05_id03', 'e2e_process_rescore_c05_id03')):
    with gzip.open(G + name + '.txt.gz', 'wt', compresslevel=9) as f: f.write(blocks(read_db('$W/' + src)))
print("rescore goldens written")
PY
