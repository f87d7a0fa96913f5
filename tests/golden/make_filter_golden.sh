#!/bin/bash
# Process-level goldens of the result filters (-c / --cov-mode / --min-seq-id) from the REAL reference binary, made like the unfiltered ones
# (make_process_golden.sh): `metaeuk predictexons` itself, built OUTSIDE the repository from a copy of the read-only reference tree; nothing of it
# is kept, only its OUTPUT DBs become fixtures (data), as '>key' blocks sorted by key:
#   e2e_process_pref_c05.txt.gz          pref_0        (prefilter, -s 5.7 -c 0.5 --cov-mode 0: the length cut of Prefiltering.cpp:856-863)
#   e2e_process_aln_c05_id03.txt.gz      search_res    (align, -c 0.5 --cov-mode 0 --min-seq-id 0.3)
#   e2e_process_calls_c05_id03.txt.gz    dp_predictions of that run
# Inputs: tests/golden/e2e_targets.txt.gz, e2e_contigs.txt.gz (createdb --shuffle 0, so keys = line numbers).  Host L2 = 2097152.  Recorded in PROVENANCE_filters.txt.
# An existing binary is used when METAEUK names one (or make_process_golden.sh left its build behind).
set -e
R=$(cd $(dirname $0)/../.. && pwd)
W=${1:-$(mktemp -d /tmp/fg.XXXXXX)}
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
mkdir tmp
$M predictexons contigsDB targetsDB calls tmp --remove-tmp-files 0 --threads 4 -s 5.7 -c 0.5 --cov-mode 0 --min-seq-id 0.3 > run.log 2>&1
python3 - <<PY
import glob, gzip, os
def read_db(base):
    if os.path.exists(base): data = open(base, 'rb').read()
    else:
        data, i = b'', 0
        while os.path.exists(base + '.%d' % i): data += open(base + '.%d' % i, 'rb').read(); i += 1
    return {int(l.split('\t')[0]): data[int(l.split('\t')[1]):int(l.split('\t')[1]) + int(l.split('\t')[2]) - 1].decode() for l in open(base + '.index')}
T, G = '$W/tmp/latest/', '$R/tests/golden/'
blocks = lambda d: "".join(">%d\n%s" % (k, d[k]) for k in sorted(d))
def write(n, t):
    with gzip.open(G + n, 'wt', compresslevel=9) as f: f.write(t)
write("e2e_process_pref_c05.txt.gz", blocks(read_db(glob.glob(T + 'tmp_search/*/pref_0.index')[0][:-6])))
write("e2e_process_aln_c05_id03.txt.gz", blocks(read_db(T + 'search_res')))
write("e2e_process_calls_c05_id03.txt.gz", blocks(read_db('$W/calls')))
# the share of alignment lines whose printed identity sits on the threshold's rounding edge (tests/test_gpu_result_filters.py leaves them out
# of its derivation check; more than 1 % of them: pick --min-seq-id 0.25 or 0.5 instead)
aln = gzip.open(G + 'e2e_process_aln.txt.gz', 'rt').read().splitlines()
recs = [l for l in aln if not l.startswith('>')]
edge = sum(1 for l in recs if l.split('\t')[2] in ('0.299', '0.300'))
print("identity on the edge (0.299 / 0.300): %d of %d unfiltered alignment lines" % (edge, len(recs)))
PY
