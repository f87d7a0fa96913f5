#!/bin/bash
# Goldens of the ORF-stage flags (--max-gaps, --forward-frames / --reverse-frames, --min-length / --max-length, --contig-end-mode,
# --reverse-fragments) from the REAL reference binary, made like the backtrace ones (make_backtrace_golden.sh): the binary is built OUTSIDE
# the repository from a copy of the read-only reference tree; nothing of it is kept, only its OUTPUT DBs become fixtures (data):
#   orf_flag_contigs.txt.gz            the input, one contig per line, generated here (seed inside)
#   orf_flag_expected_<case>.txt.gz    `extractorfs <flags>` + `translatenucs` on it: per contig '>index', then one line per fragment in key
#                                      order, "header<TAB>protein" (the block format of orf_expected.txt.gz); the cases are listed below
#   e2e_process_aln_revfrag / e2e_process_calls_revfrag / e2e_process_aa_revfrag200
#                                      search_res, dp_predictions and the first 200 entries of aa_6f_reverse of
#                                      `predictexons ... -s 5.7 --reverse-fragments 1 <REV_EXTRA>` on the e2e fixture, '>key' blocks
#   e2e_process_aln_fwd_g0 / e2e_process_calls_fwd_g0
#                                      search_res and dp_predictions of `predictexons ... -s 5.7 --reverse-frames 0 --max-gaps 0`
# The DBs of the flag cases are written directly (data 'SEQ\n\0', index, dbtype 1, header DB): createdb would refuse or rewrite some of
# the characters the input is about.  Host L2 = 2097152.  Prints the counts recorded in PROVENANCE_orf_flags.txt and checks that no case
# passes on nothing.  An existing binary is used when METAEUK names one (or another golden script left its build behind).
set -e
R=$(cd $(dirname $0)/../.. && pwd)
W=${1:-$(mktemp -d /tmp/ofg.XXXXXX)}
M=${METAEUK:-/tmp/ref-build/src/metaeuk}
# null-mode run: at the default --metaeuk-eval 0.001 / --metaeuk-tcov 0.5 the reversed fragments of the e2e fixture give no prediction at all,
# so both (honoured by the project) are loosened until dp_predictions is non-empty; recorded in the provenance file
REV_EXTRA=${REV_EXTRA:---metaeuk-eval 100 --metaeuk-tcov 0.1}
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
rng = random.Random(20261022)
STOPS = ("TAA", "TAG", "TGA")
def codon():
    while True:
        c = "".join(rng.choice("ACGT") for _ in range(3))
        if c not in STOPS: return c
def run(n): return "".join(codon() for _ in range(n))          # n stop-free codons of frame 0
def rnd(n): return "".join(rng.choice("ACGT") for _ in range(n))
def with_gaps(seq, k, ch="N"):                                   # k codons of frame 0 get one gap character
    s = list(seq)
    for c in rng.sample(range(len(seq) // 3), k): s[3 * c + rng.randrange(3)] = ch
    return "".join(s)
C = []
C += ["AC", "ACG", "ACGTA", "ANGTCA", "TAA", "NNN", "TAATAGTGA"]                     # lengths 2, 3, 5, 6; stop-only; gap-only
for k in range(4):                                               # frame-0 fragments of 30 codons with exactly k gap codons, closed by a stop
    for tail in ("", "A", "AC"):                                 # contig length = 0, 1, 2 (mod 3)
        C.append(with_gaps(run(30), k) + "TAA" + run(18) + tail)
C.append(run(20) + "TAG" + "NNN" + run(25) + "TGA" + run(16))                       # a gap codon is the first codon after a stop
C.append(run(20) + "TAG" + "ANC" + run(25))                                          # ... and the fragment runs to the contig's end
C.append(run(24) + "ACN")                                                            # a gap codon closes a frame without a stop (length = 0 mod 3)
C.append(run(24) + "NNN" + "A")                                                      # ... length = 1 mod 3
C.append("C" + run(24) + "GNT" + "AC")                                               # ... of frame 2 (strand position 1 mod 3), length = 0 mod 3
C.append(with_gaps(run(40), 2, "n") + "taa" + with_gaps(run(20), 1, "n").lower())    # lower-case n, lower-case stop
C.append(with_gaps(run(40), 1, "*") + "TAA" + with_gaps(run(22), 2, "x"))            # characters outside the IUPAC code
C.append(with_gaps(run(40), 2, "R") + "TAA" + with_gaps(run(22), 3, "Y"))            # ambiguity codes are NOT gaps
C.append(run(17) + "N" * 40 + run(17))                                               # an N run (13 gap codons in every frame)
C.append(rnd(50) + "N" * 9 + rnd(61) + "n" * 3 + rnd(70))
for n in (59, 60, 61, 121, 122, 123, 300, 301, 302, 700, 1001):                      # random contigs, some with N runs and lower case
    s = list(rnd(n))
    for _ in range(n // 150):
        p, l = rng.randrange(n), rng.randrange(1, 8)
        s[p:p + l] = "N" * len(s[p:p + l])
    if n % 2: s[n // 3:n // 2] = "".join(s[n // 3:n // 2]).lower()
    C.append("".join(s))
# longer than a scan tile of 4096 strand positions: long stop-free stretches on both sides of every multiple of 4096, single N's inside
big = []
while sum(map(len, big)) < 9000:
    big.append(with_gaps(run(rng.randrange(20, 400)), rng.randrange(0, 4)) + rng.choice(STOPS) + rnd(rng.randrange(0, 3)))
C.append("".join(big))
C.append(rnd(4099))
assert all(C) and len(C) < 64
with gzip.open(G + 'orf_flag_contigs.txt.gz', 'wt', compresslevel=9) as f: f.write("\n".join(C) + "\n")
def write_db(base, entries, dbtype):
    off = 0
    with open(base, 'wb') as d, open(base + '.index', 'w') as i:
        for k, s in enumerate(entries):
            d.write(s.encode() + b"\n\0"); i.write("%d\t%d\t%d\n" % (k, off, len(s) + 2)); off += len(s) + 2
    open(base + '.dbtype', 'wb').write(dbtype.to_bytes(4, 'little'))
write_db('flagDB', C, 1)
write_db('flagDB_h', ["f%d" % k for k in range(len(C))], 12)
def lines(n): return gzip.open(G + n, 'rt').read().splitlines()
open('targets.faa', 'w').write("".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_targets.txt.gz'))))
open('contigs.fna', 'w').write("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_contigs.txt.gz'))))
PY
CASES=(default "" nogaplimit "--max-gaps 2147483647" maxgaps0 "--max-gaps 0" maxgaps2 "--max-gaps 2"
       fwd2_rev0 "--forward-frames 2 --reverse-frames 0" fwd13_rev2 "--forward-frames 1,3 --reverse-frames 2"
       len5_40 "--min-length 5 --max-length 40" endmode0 "--contig-end-mode 0" endmode1 "--contig-end-mode 1"
       combo "--max-gaps 1 --reverse-frames 3 --contig-end-mode 1 --max-length 200")
for ((i = 0; i < ${#CASES[@]}; i += 2)); do
    c=${CASES[i]}
    # predictexons' settings (PredictExons.cpp:8-16) where the case does not say otherwise: the module's own --min-length default is 30
    base="--orf-start-mode 1 --min-length 15"
    case "${CASES[i+1]}" in *--min-length*) base="--orf-start-mode 1";; esac
    $M extractorfs flagDB nucl_$c $base ${CASES[i+1]} --threads 1 > ex_$c.log 2>&1
    $M translatenucs nucl_$c aa_$c --threads 1 > tr_$c.log 2>&1
done
$M createdb targets.faa targetsDB --shuffle 0 > /dev/null
$M createdb contigs.fna contigsDB --shuffle 0 > /dev/null
mkdir tmpR tmpF
$M predictexons contigsDB targetsDB callsR tmpR --remove-tmp-files 0 --threads 4 -s 5.7 --reverse-fragments 1 $REV_EXTRA > runR.log 2>&1
$M predictexons contigsDB targetsDB callsF tmpF --remove-tmp-files 0 --threads 4 -s 5.7 --reverse-frames 0 --max-gaps 0 > runF.log 2>&1
python3 - <<PY
import gzip, os
def read_db(base):
    if os.path.exists(base): data = open(base, 'rb').read()
    else:
        data, i = b'', 0
        while os.path.exists(base + '.%d' % i): data += open(base + '.%d' % i, 'rb').read(); i += 1
    return {int(l.split('\t')[0]): data[int(l.split('\t')[1]):int(l.split('\t')[1]) + int(l.split('\t')[2]) - 1].decode('latin-1') for l in open(base + '.index')}
G = '$R/tests/golden/'
def write(n, t):
    with gzip.open(G + n, 'wt', compresslevel=9, encoding='latin-1') as f: f.write(t)
nC = len(gzip.open(G + 'orf_flag_contigs.txt.gz', 'rt').read().splitlines())
IUPAC = set("ACGTUMRWSYKVHDB")
def gap_codons(nt):            # isGapOrN on the upper-cased characters (c & ~0x20)
    up = [chr(ord(c) & ~0x20) for c in nt.rstrip("\n")]
    return sum(1 for i in range(0, len(up) - 2, 3) if any(c == 'N' or c not in IUPAC for c in up[i:i + 3]))
def case(c):
    hdr, aa, nt = read_db('nucl_%s_h' % c), read_db('aa_%s' % c), read_db('nucl_%s' % c)
    assert sorted(hdr) == sorted(aa) == sorted(nt) == list(range(len(hdr)))
    per = [[] for _ in range(nC)]
    for k in range(len(hdr)):
        h = hdr[k].rstrip("\n")
        per[int(h.split("\t")[0])].append(h + "\t" + aa[k].rstrip("\n"))
    text = "".join(">%d\n%s" % (i, "".join(l + "\n" for l in per[i])) for i in range(nC))
    frags = {hdr[k].rstrip("\n"): gap_codons(nt[k]) for k in range(len(hdr))}
    return text, frags
text, frags = {}, {}
for c in "default nogaplimit maxgaps0 maxgaps2 fwd2_rev0 fwd13_rev2 len5_40 endmode0 endmode1 combo".split():
    text[c], frags[c] = case(c)
assert text['default'] == text['nogaplimit']
hist = {}
for g in frags['default'].values(): hist[g] = hist.get(g, 0) + 1
print("default: %d fragments; gap codons per fragment: %s" % (len(frags['default']), sorted(hist.items())))
assert all(hist.get(g, 0) > 0 for g in (0, 1, 2, 3))
for c in "maxgaps0 maxgaps2 fwd2_rev0 fwd13_rev2 len5_40 endmode0 endmode1 combo".split():
    assert frags[c] and text[c] != text['default'], c            # no case passes on nothing
    write('orf_flag_expected_%s.txt.gz' % c, text[c])
    print("%s: %d fragments, %d of them with a gap codon" % (c, len(frags[c]), sum(1 for g in frags[c].values() if g)))
kept = sum(1 for g in frags['maxgaps2'].values() if g > 0)
dropped = len(set(frags['nogaplimit']) - set(frags['maxgaps2']))
assert kept > 0 and dropped > 0
assert set(frags['maxgaps2']) == {h for h, g in frags['default'].items() if g <= 2}
print("--max-gaps 2 keeps %d fragments with a gap codon and drops %d that --max-gaps 2147483647 keeps" % (kept, dropped))
blocks = lambda d: "".join(">%d\n%s" % (k, d[k]) for k in sorted(d))
for tag, tmp, calls in (("revfrag", "tmpR", "callsR"), ("fwd_g0", "tmpF", "callsF")):
    aln, pred = read_db('$W/%s/latest/search_res' % tmp), read_db('$W/' + calls)
    write("e2e_process_aln_%s.txt.gz" % tag, blocks(aln))
    write("e2e_process_calls_%s.txt.gz" % tag, blocks(pred))
    print("%s: %d alignment records, %d prediction lines in %d contigs" % (tag, sum(len(b.splitlines()) for b in aln.values()),
          sum(len(b.splitlines()) for b in pred.values()), sum(1 for b in pred.values() if b)))
    assert any(pred.values()), tag
rev = read_db('$W/tmpR/latest/aa_6f_reverse')
write("e2e_process_aa_revfrag200.txt.gz", blocks({k: rev[k] for k in sorted(rev)[:200]}))
print("aa_6f_reverse: %d entries, the first 200 kept; REV_EXTRA = '%s'" % (len(rev), "$REV_EXTRA"))
PY
