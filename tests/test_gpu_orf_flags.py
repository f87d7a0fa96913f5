"""The ORF-stage flags on the GPU (mk_orf.hip): --max-gaps, --forward-frames / --reverse-frames, --min-length / --max-length,
--contig-end-mode and --reverse-fragments against the output of the real `extractorfs` + `translatenucs` and of the real
`predictexons` (tests/golden/PROVENANCE_orf_flags.txt), against the host twin on seeded contigs, and through the commands."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from test_orf_flags_host import CASES, GOLD, INT_MAX, lines, orf_text, params_of, text

pytestmark = pytest.mark.gpu
L2 = 2097152                                       # tests/golden/PROVENANCE.txt

# the flags each fixture case was made with (tests/golden/make_orf_flag_golden.sh)
ARGV = {
    "maxgaps0": ["--max-gaps", "0"],
    "maxgaps2": ["--max-gaps", "2"],
    "fwd2_rev0": ["--forward-frames", "2", "--reverse-frames", "0"],
    "fwd13_rev2": ["--forward-frames", "1,3", "--reverse-frames", "2"],
    "len5_40": ["--min-length", "5", "--max-length", "40"],
    "endmode0": ["--contig-end-mode", "0"],
    "endmode1": ["--contig-end-mode", "1"],
    "combo": ["--max-gaps", "1", "--reverse-frames", "3", "--contig-end-mode", "1", "--max-length", "200"],
}


def _write_seq_db(base, seqs, dbtype=0):
    off = 0
    with open(base, "wb") as d, open(base + ".index", "w") as i:
        for k, s in enumerate(seqs):
            d.write(s.encode("latin-1") + b"\n\0")
            i.write("%d\t%d\t%d\n" % (k, off, len(s) + 2))
            off += len(s) + 2
    with open(base + ".dbtype", "wb") as t:
        t.write(dbtype.to_bytes(4, "little"))


def _read_db(base):
    data = open(base, "rb").read()
    out = {}
    for line in open(base + ".index"):
        k, o, l = line.split("\t")
        out[int(k)] = data[int(o):int(o) + int(l) - 1].decode("latin-1")
    return out


def _same_orfs(a, b):
    assert a.n == b.n and a.orfs.tobytes() == b.orfs.tobytes() and np.array_equal(a.aa_off, b.aa_off) and a.aa == b.aa


@pytest.fixture(scope="module")
def flag_contigs():
    return lines("orf_flag_contigs.txt.gz")


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_reproduces_the_reference(gpu_api, flag_contigs, case):
    o = gpu_api.Orfs(flag_contigs, params=params_of(gpu_api, case))
    assert o.n > 0 and orf_text(o, len(flag_contigs)) == text("orf_flag_expected_%s.txt.gz" % case)
    _same_orfs(o, gpu_api.Orfs(flag_contigs, params=params_of(gpu_api, case), host=True))


def test_device_defaults_are_unchanged(gpu_api, flag_contigs):
    """mk_extract_orfs = mk_extract_orfs_ex with the defaults, on the old and the new fixture input; an explicit gap limit nothing exceeds
    (the counting walk) gives the same fragments as no limit (the plain walk)"""
    api = gpu_api
    old = lines("orf_contigs.txt.gz")
    assert orf_text(api.Orfs(old), len(old)) == text("orf_expected.txt.gz")
    plain = api.Orfs(flag_contigs)
    _same_orfs(plain, api.Orfs(flag_contigs, host=True))
    _same_orfs(plain, api.Orfs(flag_contigs, params=api.default_orf_params(max_gap_codons=INT_MAX - 1)))
    none = api.Orfs(flag_contigs, params=api.default_orf_params(forward_frames=0, reverse_frames=0))
    assert none.n == 0 and none.queries().n == 0


def test_device_equals_the_twin_on_seeded_contigs(gpu_api):
    """synthetic contigs with N runs, lower case and a junk character: a dozen seeded parameter combinations, device against host twin"""
    from metaeuk_amd import synth
    api = gpu_api
    _, founders = synth.make_targets(300, 9)
    rs = np.random.RandomState(44)
    contigs = []
    for c in synth.make_contigs(25, founders, 9):
        s = np.array(list("ACGT"))[np.asarray(c)]
        for _ in range(max(1, len(s) // 400)):                       # N runs of 1 .. 30 over ~1.5 % of the bases
            p, n = rs.randint(len(s)), rs.randint(1, 31)
            s[p:p + n] = "N" if rs.rand() < 0.8 else "n"
        if rs.rand() < 0.3:
            s[rs.randint(len(s))] = "*"
        contigs.append("".join(s))
    contigs += ["AC", "", "NNNTAANNN"]
    seen = set()
    for _ in range(12):
        kw = dict(min_codons=int(rs.choice([1, 5, 15, 40])), max_codons=int(rs.choice([20, 100, 32734, 65535])),
                  max_gap_codons=int(rs.choice([0, 1, 2, 5, INT_MAX])), forward_frames=int(rs.randint(0, 8)), reverse_frames=int(rs.randint(0, 8)),
                  contig_end_mode=int(rs.randint(0, 3)), reverse_fragments=int(rs.randint(0, 2)))
        dev = api.Orfs(contigs, params=api.default_orf_params(**kw))
        _same_orfs(dev, api.Orfs(contigs, params=api.default_orf_params(**kw), host=True))
        seen.add(dev.n > 0)
    assert True in seen


def test_reversed_orfs_feed_the_search(gpu_api):
    """--reverse-fragments: the codes the translate kernel wrote back to front search like the same strings handed in as a query batch"""
    from metaeuk_amd import synth
    api = gpu_api
    targets, founders = synth.make_targets(300, 9)
    tstr = [synth.codes_to_str(t) for t in targets]
    contigs = ["".join("ACGT"[x] for x in c) for c in synth.make_contigs(25, founders, 9)]
    fwd = api.Orfs(contigs)
    o = api.Orfs(contigs, params=api.default_orf_params(reverse_fragments=1))
    assert o.n == fwd.n and [o.protein(k) for k in range(o.n)] == [fwd.protein(k)[::-1] for k in range(o.n)]
    params = api.default_params()
    db = api.TargetDB(tstr, params)
    q1 = o.queries(params)
    (h1, ho1), (a1, ao1) = api.search(db, q1)
    q2 = api.Queries([o.protein(k) for k in range(o.n)], params)
    (h2, ho2), (a2, ao2) = api.search(db, q2)
    assert np.array_equal(np.asarray(ho1), np.asarray(ho2)) and h1.tobytes() == h2.tobytes()
    assert np.array_equal(np.asarray(ao1), np.asarray(ao2))
    n = int(ao1[-1])
    assert api.format_alignments(a1, 0, n) == api.format_alignments(a2, 0, n)
    # the forward fragments find their homologs, the reversed ones (the null model) almost nothing
    (_, _), (_, aof) = api.search(db, fwd.queries(params))
    assert int(aof[-1]) > 20 and n < int(aof[-1])


@pytest.mark.parametrize("case", sorted(CASES))
def test_cli_extractorfs_with_flags(gpu_api, flag_contigs, tmp_path, case):
    from metaeuk_amd import build
    t = str(tmp_path) + "/"
    _write_seq_db(t + "contigs", flag_contigs, 1)
    argv = ARGV[case] if "--min-length" in ARGV[case] else ["--min-length", "15"] + ARGV[case]
    subprocess.check_call([build.BIN, "extractorfs", t + "contigs", t + "nucl_6f", "--orf-start-mode", "1", "--contig-start-mode", "2",
                           "--use-all-table-starts", "1", "--threads", "4", "--aa-sibling", "aa_6f"] + argv, stderr=subprocess.DEVNULL)
    hdr, aa, nuc = _read_db(t + "nucl_6f_h"), _read_db(t + "aa_6f"), _read_db(t + "nucl_6f")
    per = [[] for _ in flag_contigs]
    assert sorted(hdr) == sorted(aa) == sorted(nuc) == list(range(len(hdr)))
    for k in range(len(hdr)):
        h = hdr[k].rstrip("\n")
        per[int(h.split("\t")[0])].append(h + "\t" + aa[k].rstrip("\n"))
        assert len(nuc[k]) == 3 * len(aa[k].rstrip("\n")) + 1
    assert "".join(">%d\n%s" % (i, "".join(l + "\n" for l in per[i])) for i in range(len(per))) == text("orf_flag_expected_%s.txt.gz" % case)


@pytest.mark.parametrize("tag,flags,orf_kw", [
    ("revfrag", ["--reverse-fragments", "1", "--metaeuk-eval", "100", "--metaeuk-tcov", "0.1"], dict(reverse_fragments=1)),
    ("fwd_g0", ["--reverse-frames", "0", "--max-gaps", "0"], dict(reverse_frames=0, max_gap_codons=0)),
])
def test_predictexons_equals_the_real_process(gpu_api, tmp_path, tag, flags, orf_kw):
    """search_res (through the library: fragments -> query batch -> search) and dp_predictions (through the command) of the real binary's
    `predictexons -s 5.7 <flags>` on the e2e fixture, byte for byte"""
    from metaeuk_amd import build
    api = gpu_api
    targets, contigs = lines("e2e_targets.txt.gz"), lines("e2e_contigs.txt.gz")
    params = api.default_params()
    params.host_l2_bytes = L2
    params.sensitivity = 5.7
    db = api.TargetDB(targets, params)
    o = api.Orfs(contigs, params=api.default_orf_params(**orf_kw))
    q = o.queries(params)
    _, (alns, aoff) = api.search(db, q)
    got = "".join(">%d\n%s" % (k, api.format_alignments(alns, int(aoff[k]), int(aoff[k + 1]))) for k in range(o.n))
    want = text("e2e_process_aln_%s.txt.gz" % tag)
    assert want.count("\t") > 1000 and got == want
    t = str(tmp_path) + "/"
    _write_seq_db(t + "targets", targets)
    _write_seq_db(t + "contigs", contigs, 1)
    subprocess.check_call([build.BIN, "predictexons", t + "contigs", t + "targets", t + "calls", t + "tmp", "--threads", "4", "--ref-l2-bytes", str(L2),
                           "-s", "5.7"] + flags, stderr=subprocess.DEVNULL)
    calls = _read_db(t + "calls")
    want = text("e2e_process_calls_%s.txt.gz" % tag)
    assert want.count("\t") > 500 and "".join(">%d\n%s" % (k, calls[k]) for k in sorted(calls)) == want


def test_corners_still_refused_by_name(gpu_api, flag_contigs, tmp_path):
    from metaeuk_amd import build
    t = str(tmp_path) + "/"
    _write_seq_db(t + "contigs", flag_contigs, 1)
    _write_seq_db(t + "targets", lines("e2e_targets.txt.gz")[:50])
    (tmp_path / "profDB").write_bytes(gzip.open(os.path.join(GOLD, "prof_db.bin.gz"), "rb").read())
    (tmp_path / "profDB.index").write_text(open(os.path.join(GOLD, "prof_db.index")).read())
    (tmp_path / "profDB.dbtype").write_bytes((2).to_bytes(4, "little"))
    bad = [["--contig-start-mode", "1"], ["--orf-start-mode", "0"], ["--translation-table", "4"], ["--add-orf-stop", "1"]]
    for n, flags in enumerate(bad):
        for cmd in (["extractorfs", t + "contigs", t + "x%d" % n], ["predictexons", t + "contigs", t + "targets", t + "y%d" % n, t + "tmp"]):
            r = subprocess.run([build.BIN] + cmd + flags, capture_output=True)
            assert r.returncode != 0 and flags[0].encode() in r.stderr, (cmd[0], flags, r.stderr)
            assert not os.path.exists(cmd[-1 if cmd[0] == "extractorfs" else -2] + ".dbtype")
    r = subprocess.run([build.BIN, "predictexons", t + "contigs", t + "profDB", t + "z", t + "tmp", "--reverse-fragments", "1"], capture_output=True)
    assert r.returncode != 0 and b"--reverse-fragments" in r.stderr and not os.path.exists(t + "z.dbtype")
    for flags in (["--max-length", "65536"], ["--contig-end-mode", "3"], ["--max-gaps", "x"]):
        r = subprocess.run([build.BIN, "extractorfs", t + "contigs", t + "w"] + flags, capture_output=True)
        assert r.returncode != 0 and flags[0].encode() in r.stderr and not os.path.exists(t + "w.dbtype")
