#!/bin/bash
# Goldens of the genetic code and the ORF start modes (--translation-table, --orf-start-mode, --use-all-table-starts, --contig-start-mode,
# --add-orf-stop) from the REAL reference binary, made like the ORF-flag ones (make_orf_flag_golden.sh): the binary is built OUTSIDE the
# repository from a copy of the read-only reference tree, with -DHAVE_AVX2=1 (the build whose start/stop comparison looks at all eight
# codon slots, Orf.cpp:201-226); nothing of it is kept, only its OUTPUT DBs become fixtures (data):
#   orf_code_contigs.txt.gz            the input, one contig per line, generated here (seed inside)
#   orf_code_expected_<case>.txt.gz    `extractorfs --min-length 15 <flags>` + `translatenucs <flags>` on it: per contig '>index', then one line
#                                      per fragment in key order, "header<TAB>protein" (the block format of orf_expected.txt.gz)
#   orf_code_tables.txt.gz             one nucleotide entry with all 15^3 codons over ACMGRSVTWYHKDBN through `translatenucs
#                                      --translation-table T` for each of the 25 codes: one line "T<TAB>protein" per code
#   orf_code_starts.txt.gz             the start set of every code: the header DB of `extractorfs --min-length 15 --orf-start-mode 2
#                                      --use-all-table-starts 1 --translation-table T` on the input (mode 2 moves a fragment's begin to every
#                                      start codon, so a wrong member of the set moves some header): per code '#T', then the headers in key order
#   e2e_process_aln_<tag> / e2e_process_calls_<tag>
#                                      search_res and dp_predictions of `predictexons ... -s 5.7 <flags>` on the e2e fixture, '>key' blocks;
#                                      tags t6 (--translation-table 6), mode0 (--orf-start-mode 0).  There is no such run with
#                                      --add-orf-stop 1: the reference's predictexons takes the flag out of its parameter list
#                                      (src/commons/LocalParameters.h:110) and answers "Unrecognized parameter"; that answer is checked here
# The DBs of the cases are written directly (data 'SEQ\n\0', index, dbtype 1, header DB): createdb would refuse or rewrite some of the
# characters the input is about.  Host L2 = 2097152.  Prints the counts recorded in PROVENANCE_orf_codes.txt and checks that no case
# passes on nothing.  An existing binary is used when METAEUK names one (or another golden script left its build behind).
set -e
R=$(cd $(dirname $0)/../.. && pwd)
W=${1:-$(mktemp -d /tmp/ocg.XXXXXX)}
M=${METAEUK:-/tmp/ref-build/src/metaeuk}
# a process run whose dp_predictions is empty at the default --metaeuk-eval / --metaeuk-tcov gets both loosened like REV_EXTRA of
# make_orf_flag_golden.sh; which run needed it is printed (and recorded in the provenance file)
LOOSE=${LOOSE:---metaeuk-eval 100 --metaeuk-tcov 0.1}
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
rng = random.Random(20261021)
STOPS = ("TAA", "TAG", "TGA", "AGA", "AGG", "TCA", "TTA")          # a stop in at least one genetic code
STARTS = ("ATG", "TTG", "CTG", "GTG", "ATT", "ATC", "ATA")         # a start in at least one genetic code (TTA is both lists' business: code 4 / 23)
SPECIAL = set(STOPS) | set(STARTS)
def codon(avoid):
    while True:
        c = "".join(rng.choice("ACGT") for _ in range(3))
        if c not in avoid: return c
def run(n): return "".join(codon(SPECIAL) for _ in range(n))       # n codons of frame 0 that are neither a stop nor a start in any code
def run1(n): return "".join(codon(STOPS[:3]) for _ in range(n))    # n codons without a stop of code 1 (start codons as they fall)
def rnd(n): return "".join(rng.choice("ACGT") for _ in range(n))
C = []
C += ["AC", "ACG", "ACGTA", "ATGTCA", "TAA", "NNN", "ATG", "ATGTAA"]                # lengths 2, 3, 5, 6; stop-only; gap-only; start-only
for i, s in enumerate(STOPS):                                       # frames whose only candidate stop is s; contig length = 0, 1, 2 (mod 3)
    C.append(run(20) + s + run(18) + ("", "A", "AC")[i % 3])
for i, s in enumerate(STARTS):                                      # fragments that begin with each start codon, after a stop and at a contig's begin
    C.append(run(6) + "TAA" + run(3) + s + run(20) + "TAG" + run(16) + ("", "C", "CA")[i % 3])
C.append("ATG" + run(22) + "TGA" + "TTG" + run(19))
C.append(run(5) + "TAA" + run(4) + "ATG" + run(17) + "ATG" + run(18) + "TAG" + run(16))        # two starts in one stop-free stretch: modes 0 and 2 differ
C.append(run(4) + "ATG" + run(17) + "ATG" + run(16) + "TAA" + run(15) + "A")                    # ... before the frame's first stop
C.append(run(20) + "TAA" + run(17) + "ATG" + "TAA" + run(20) + "ATG" + "TGA" + run(3) + "ATG" + run(15))   # a start directly before a stop
C.append(run(41) + "GT")                                                                         # a stop-free frame without a start codon
C.append("TAA" + run(20) + "ATG" + run(20) + "TAG" + run(17))                                    # the frame's first codon is a stop
C.append(run(16) + "TAA" + run(2) + "ATG" + run(16) + "TAG" + run(20) + "TGA" + run(16) + "ATG" + run(15))  # a start between two stops, none between the next two
C.append((run(16) + "taa" + run(2) + "atg" + run(16).lower() + "tAg" + run(20) + "tga" + run(16) + "aTG" + run(15)) + "c")  # lower-case starts and stops
# the end-star rule: UAA (capital U) and TAR are no stops for the scan and translate to '*'; here they are the last codon before a real stop
C.append(run(20) + "UAA" + "TAA" + run(16) + "TAR" + "TGA" + "ATG" + run(18) + "UAG" + "TAG" + run(16))
C.append(run(3) + "TAA" + "ATG" + run(20) + "TAR" + "TAA" + run(2) + "ATG" + run(17) + "uaa" + "taa" + run(15))
# gap codons before and after a start codon inside one stretch (the count begins anew at the start in modes 0 and 2)
C.append(run(3) + "TAA" + run(3) + "ANC" + run(2) + "ATG" + run(8) + "NNN" + run(10) + "TAA" + run(15))       # 1 gap before, 1 after
C.append(run(3) + "TAA" + run(2) + "ATG" + run(6) + "NNN" + run(6) + "CNG" + run(8) + "TAG" + run(15))         # 2 gaps after the start
C.append(run(3) + "TAA" + run(2) + "ATG" + run(3) + "NNN" + run(3) + "ATG" + run(16) + "TAA" + run(15))        # a gap between two starts
C.append(run(2) + "GNN" + run(3) + "ATG" + run(16) + "ANA" + "TGA" + run(15) + "NN")                             # ... before the frame's first stop
C.append(run(17) + "N" * 40 + run(17))                                                           # an N run (13 gap codons in every frame)
C.append(rnd(50) + "N" * 9 + rnd(61) + "n" * 3 + rnd(70))
for n in (59, 60, 61, 121, 122, 123, 300, 301, 302, 700, 1001):                                  # random contigs, some with N runs and lower case
    s = list(rnd(n))
    for _ in range(n // 150):
        p, l = rng.randrange(n), rng.randrange(1, 8)
        s[p:p + l] = "N" * len(s[p:p + l])
    if n % 2: s[n // 3:n // 2] = "".join(s[n // 3:n // 2]).lower()
    C.append("".join(s))
# longer than a scan tile of 4096 strand positions: stop-free stretches (of code 1; start codons as they fall) across every multiple of 4096
while True:
    big, cuts = [], []
    while sum(map(len, big)) < 9000:
        big.append(run1(rng.randrange(20, 400)) + rng.choice(STOPS[:3]) + rnd(rng.randrange(0, 3)))
        cuts.append(sum(map(len, big)))
    if all(min(abs(c - m) for c in cuts) > 60 for m in (4096, 8192)): break
C.append("".join(big))
C.append(rnd(4099))
assert all(C) and len(C) < 64
with gzip.open(G + 'orf_code_contigs.txt.gz', 'wt', compresslevel=9) as f: f.write("\n".join(C) + "\n")
def write_db(base, entries, dbtype):
    off = 0
    with open(base, 'wb') as d, open(base + '.index', 'w') as i:
        for k, s in enumerate(entries):
            d.write(s.encode() + b"\n\0"); i.write("%d\t%d\t%d\n" % (k, off, len(s) + 2)); off += len(s) + 2
    open(base + '.dbtype', 'wb').write(dbtype.to_bytes(4, 'little'))
write_db('codeDB', C, 1)
write_db('codeDB_h', ["f%d" % k for k in range(len(C))], 12)
A = "ACMGRSVTWYHKDBN"
write_db('codonDB', ["".join(a + b + c for a in A for b in A for c in A)], 1)
write_db('codonDB_h', ["codons"], 12)
def lines(n): return gzip.open(G + n, 'rt').read().splitlines()
open('targets.faa', 'w').write("".join(">t%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_targets.txt.gz'))))
open('contigs.fna', 'w').write("".join(">c%d\n%s\n" % (i, s) for i, s in enumerate(lines('e2e_contigs.txt.gz'))))
PY
# case, extractorfs flags, translatenucs flags (the reference's extractorfs does not know --add-orf-stop; both take --translation-table)
CASES=(plain "" ""
       t6 "--translation-table 6" "--translation-table 6"
       t2 "--translation-table 2" "--translation-table 2"
       t22 "--translation-table 22" "--translation-table 22"
       mode0 "--orf-start-mode 0" ""
       mode2 "--orf-start-mode 2" ""
       mode0_cs1 "--orf-start-mode 0 --contig-start-mode 1" ""
       mode2_cs0 "--orf-start-mode 2 --contig-start-mode 0" ""
       mode0_gaps1 "--orf-start-mode 0 --max-gaps 1" ""
       mode1_gaps1 "--max-gaps 1" ""
       mode2_gaps1 "--orf-start-mode 2 --max-gaps 1" ""
       t4_mode0_all "--translation-table 4 --orf-start-mode 0 --use-all-table-starts 1" "--translation-table 4"
       t11_mode2_all_combo "--translation-table 11 --orf-start-mode 2 --use-all-table-starts 1 --reverse-frames 2 --contig-end-mode 1" "--translation-table 11"
       addstop "" "--add-orf-stop 1"
       addstop_mode0_t6 "--orf-start-mode 0 --translation-table 6" "--add-orf-stop 1 --translation-table 6")
for ((i = 0; i < ${#CASES[@]}; i += 3)); do
    c=${CASES[i]}
    base="--orf-start-mode 1 --min-length 15"
    case "${CASES[i+1]}" in *--orf-start-mode*) base="--min-length 15";; esac
    $M extractorfs codeDB nucl_$c $base ${CASES[i+1]} --threads 1 > ex_$c.log 2>&1
    $M translatenucs nucl_$c aa_$c ${CASES[i+2]} --threads 1 > tr_$c.log 2>&1
done
for T in 1 2 3 4 5 6 9 10 11 12 13 14 15 16 21 22 23 24 25 26 27 28 29 30 31; do
    $M translatenucs codonDB codons_$T --translation-table $T --threads 1 > trc_$T.log 2>&1
    $M extractorfs codeDB starts_$T --min-length 15 --orf-start-mode 2 --use-all-table-starts 1 --translation-table $T --threads 1 > exs_$T.log 2>&1
done
$M createdb targets.faa targetsDB --shuffle 0 > /dev/null
$M createdb contigs.fna contigsDB --shuffle 0 > /dev/null
PROC=(t6 "--translation-table 6" mode0 "--orf-start-mode 0")
for ((i = 0; i < ${#PROC[@]}; i += 2)); do
    t=${PROC[i]}
    mkdir tmp_$t
    $M predictexons contigsDB targetsDB calls_$t tmp_$t --remove-tmp-files 0 --threads 4 -s 5.7 ${PROC[i+1]} > run_$t.log 2>&1
    if ! awk '$3 > 1' calls_$t.index | grep -q .; then
        echo "process run $t: no prediction at the default --metaeuk-eval / --metaeuk-tcov, run again with $LOOSE"
        rm -rf tmp_$t calls_$t*; mkdir tmp_$t
        $M predictexons contigsDB targetsDB calls_$t tmp_$t --remove-tmp-files 0 --threads 4 -s 5.7 ${PROC[i+1]} $LOOSE > run_$t.log 2>&1
    fi
done
mkdir tmp_addstop
if $M predictexons contigsDB targetsDB calls_addstop tmp_addstop --threads 4 -s 5.7 --add-orf-stop 1 > run_addstop.log 2>&1; then
    echo "the reference's predictexons took --add-orf-stop: add the process fixture"; exit 1
fi
grep -q 'Unrecognized parameter "--add-orf-stop"' run_addstop.log
echo "predictexons --add-orf-stop 1: refused by the reference (Unrecognized parameter), no process fixture"
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
contigs = gzip.open(G + 'orf_code_contigs.txt.gz', 'rt').read().splitlines()
nC = len(contigs)
COMP = dict(zip("ACGTUMRWSYKVHDBNacgtumrwsykvhdbn", "TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn"))
IUPAC = set("ACGTUMRWSYKVHDB")
def case(c):
    hdr, aa, nt = read_db('nucl_%s_h' % c), read_db('aa_%s' % c), read_db('nucl_%s' % c)
    assert sorted(hdr) == sorted(aa) == sorted(nt) == list(range(len(hdr)))
    per = [[] for _ in range(nC)]
    frags = {}
    for k in range(len(hdr)):
        h = hdr[k].rstrip("\n")
        per[int(h.split("\t")[0])].append(h + "\t" + aa[k].rstrip("\n"))
        frags[h] = (aa[k].rstrip("\n"), nt[k].rstrip("\n"))
    return "".join(">%d\n%s" % (i, "".join(l + "\n" for l in per[i])) for i in range(nC)), frags
def parts(h):                       # header -> contig, closing end (strand, last nucleotide), codons, incomplete-start / -end
    f = h.split("\t")
    sign = '+' if '+' in f[1] else '-'
    a, l = f[1].split(sign)
    flags = int(f[2]) if len(f) > 2 else 0
    to = int(a) + int(l) if sign == '+' else int(a) - int(l)
    return int(f[0]), (sign, to), (int(l) + 1) // 3, flags & 1, (flags >> 1) & 1
def gap_codons(nt):
    up = [chr(ord(c) & ~0x20) for c in nt]
    return [any(c == 'N' or c not in IUPAC for c in up[i:i + 3]) for i in range(0, len(up) - 2, 3)]
names = "plain t6 t2 t22 mode0 mode2 mode0_cs1 mode2_cs0 mode0_gaps1 mode1_gaps1 mode2_gaps1 t4_mode0_all t11_mode2_all_combo addstop addstop_mode0_t6".split()
text, frags = {}, {}
for c in names: text[c], frags[c] = case(c)
print("%d contigs, %d nucleotides; plain (--orf-start-mode 1 --min-length 15): %d fragments" % (nC, sum(map(len, contigs)), len(frags['plain'])))
for c in names:
    if c in ('plain', 'mode1_gaps1'): continue
    assert frags[c] and text[c] != text['plain'], c                 # no case passes on nothing
    write('orf_code_expected_%s.txt.gz' % c, text[c])
    print("%s: %d fragments, %d with an incomplete start, %d with an incomplete end" % (c, len(frags[c]),
          sum(parts(h)[3] for h in frags[c]), sum(parts(h)[4] for h in frags[c])))
assert text['mode0'] != text['mode2']
both = set(frags['mode0']) & set(frags['mode2'])
print("mode0 / mode2: %d headers in both, %d only in mode 0, %d only in mode 2" % (len(both), len(set(frags['mode0']) - both), len(set(frags['mode2']) - both)))
assert set(frags['mode0']) - both and set(frags['mode2']) - both
for sub, full, keep in (('mode0_cs1', 'mode0', 0), ('mode2_cs0', 'mode2', 1)):
    a, b = set(frags[sub].items()), set(frags[full].items())
    assert a and a < b, sub
    assert a == {(h, v) for h, v in b if parts(h)[3] == keep}, sub
    print("%s: %d of the %d fragments of %s (those with incomplete start = %d)" % (sub, len(a), len(b), full, keep))
# the gap limit in mode 0 counts from the farthest start
end = lambda h: (parts(h)[0],) + parts(h)[1]
dropped0 = {end(h) for h in set(frags['mode0']) - set(frags['mode0_gaps1'])}
dropped1 = {end(h) for h in set(frags['plain']) - set(frags['mode1_gaps1'])}
assert set(frags['mode0_gaps1']) < set(frags['mode0']) and dropped0 & dropped1
def gaps_before_start(h):           # gap codons of the frame between the previous stop (as --orf-start-mode 1 sees it) and this fragment's start
    for h1, (aa1, nt1) in frags['plain'].items():
        if end(h1) == end(h) and parts(h1)[2] > parts(h)[2]: return sum(gap_codons(nt1)[:parts(h1)[2] - parts(h)[2]])
    return 0
kept_gap_before = [h for h in frags['mode0_gaps1'] if gaps_before_start(h) > 0]
kept_only_mode0 = [h for h in kept_gap_before if end(h) in dropped1]
assert kept_gap_before and kept_only_mode0
print("mode0_gaps1 drops %d fragments of mode0, %d of them end where --orf-start-mode 1 --max-gaps 1 drops one too; it keeps %d fragments with a gap codon "
      "between the previous stop and their start, %d of them end where --orf-start-mode 1 --max-gaps 1 drops its fragment" %
      (len(dropped0), len(dropped0 & dropped1), len(kept_gap_before), len(kept_only_mode0)))
assert set(frags['mode2_gaps1']) < set(frags['mode2'])
print("mode2_gaps1 drops %d fragments of mode2" % (len(frags['mode2']) - len(frags['mode2_gaps1'])))
# --add-orf-stop
for c, nostar in (('addstop', 'plain'), ('addstop_mode0_t6', None)):
    hist, kept_end = {}, 0
    for h, (aa, nt) in frags[c].items():
        _, _, codons, inc_s, inc_e = parts(h)
        stars = len(aa) - codons
        hist[stars] = hist.get(stars, 0) + 1
        assert 0 <= stars <= 2 and (aa[0] == '*') >= (not inc_s)
        if not inc_e and stars == (0 if inc_s else 1):
            assert aa[-1] == '*'; kept_end += 1
    print("%s: fragments with 0 / 1 / 2 added stars: %d / %d / %d; %d with a complete end and NO trailing star added (the last codon is '*' already)" %
          (c, hist.get(0, 0), hist.get(1, 0), hist.get(2, 0), kept_end))
    if c == 'addstop':
        assert all(hist.get(s, 0) > 0 for s in (0, 1, 2)) and kept_end > 0
        assert list(frags[c]) == list(frags[nostar])
firsts = {}
for h, (aa, nt) in frags['t4_mode0_all'].items():
    if not parts(h)[3]: firsts[nt[:3].upper()] = firsts.get(nt[:3].upper(), 0) + 1
print("t4_mode0_all: first codons of the fragments with a complete start: %s" % sorted(firsts.items()))
assert len(firsts) >= 5
rows = []
for T in (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31):
    aa = read_db('codons_%d' % T)[0].rstrip("\n")
    assert len(aa) == 15 ** 3
    rows.append("%d\t%s\n" % (T, aa))
write('orf_code_tables.txt.gz', "".join(rows))
print("orf_code_tables: %d codes x %d codons, %d different tables" % (len(rows), 15 ** 3, len({r.split("\t")[1] for r in rows})))
starts = {}
for T in (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31):
    hdr = read_db('starts_%d_h' % T)
    assert hdr and sorted(hdr) == list(range(len(hdr)))
    starts[T] = "".join(hdr[k] for k in range(len(hdr)))
write('orf_code_starts.txt.gz', "".join("#%d\n%s" % (T, starts[T]) for T in sorted(starts)))
print("orf_code_starts: fragments per code %s; %d different header lists" % (", ".join("%d: %d" % (T, starts[T].count("\n")) for T in sorted(starts)), len(set(starts.values()))))
blocks = lambda d: "".join(">%d\n%s" % (k, d[k]) for k in sorted(d))
for tag in ("t6", "mode0"):
    aln, pred = read_db('$W/tmp_%s/latest/search_res' % tag), read_db('$W/calls_' + tag)
    write("e2e_process_aln_%s.txt.gz" % tag, blocks(aln))
    write("e2e_process_calls_%s.txt.gz" % tag, blocks(pred))
    print("%s: %d alignment records, %d prediction lines in %d contigs" % (tag, sum(len(b.splitlines()) for b in aln.values()),
          sum(len(b.splitlines()) for b in pred.values()), sum(1 for b in pred.values() if b)))
    assert any(pred.values()), tag
PY
