"""The genetic code, the ORF start modes and --add-orf-stop on the GPU (mk_orf.hip: orf_mark_modes_kernel / orf_write_modes_kernel and the
star-aware translate kernel) against the output of the real `extractorfs` + `translatenucs` and of the real `predictexons`
(tests/golden/PROVENANCE_orf_codes.txt) and against the host twin on seeded contigs, through the library."""
import numpy as np
import pytest

from test_gpu_orf_flags import L2, _same_orfs
from test_gpu_parity import _prediction_text
from test_orf_codes_host import CASES, CODES, all_codons, params_of, starts_params
from test_orf_flags_host import INT_MAX, lines, orf_text, text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def code_contigs():
    return lines("orf_code_contigs.txt.gz")


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_reproduces_the_reference(gpu_api, code_contigs, case):
    o = gpu_api.Orfs(code_contigs, params=params_of(gpu_api, case))
    assert o.n > 0 and orf_text(o, len(code_contigs)) == text("orf_code_expected_%s.txt.gz" % case)
    _same_orfs(o, gpu_api.Orfs(code_contigs, params=params_of(gpu_api, case), host=True))


def test_device_translates_every_codon_under_every_code(gpu_api):
    """the 15^3 IUPAC codons in one frame, every code: device = twin (the twin is pinned to the real translatenucs by the CPU suite)"""
    api = gpu_api
    for t in CODES:
        kw = dict(translation_table=t, min_codons=1, forward_frames=1, reverse_frames=0)
        _same_orfs(api.Orfs([all_codons()], params=api.default_orf_params(**kw)), api.Orfs([all_codons()], params=api.default_orf_params(**kw), host=True))


def test_device_has_the_start_set_of_every_code(gpu_api, code_contigs):
    """mode 2 with all table starts, every code: device = twin (the twin is pinned to the real extractorfs by orf_code_starts in the CPU suite)"""
    for t in CODES:
        _same_orfs(gpu_api.Orfs(code_contigs, params=starts_params(gpu_api, t)), gpu_api.Orfs(code_contigs, params=starts_params(gpu_api, t), host=True))


def test_device_defaults_and_the_general_walk_agree(gpu_api, code_contigs):
    """the default call on the new input is the twin's, and genetic code 11 (stops and residues of code 1) through the kernels of the
    general rule gives the same records as the default kernels, with and without a gap limit"""
    api = gpu_api
    plain = api.Orfs(code_contigs)
    _same_orfs(plain, api.Orfs(code_contigs, host=True))
    _same_orfs(plain, api.Orfs(code_contigs, params=api.default_orf_params(translation_table=11)))
    for kw in (dict(max_gap_codons=0), dict(max_gap_codons=2, contig_end_mode=1, min_codons=1)):
        _same_orfs(api.Orfs(code_contigs, params=api.default_orf_params(**kw)), api.Orfs(code_contigs, params=api.default_orf_params(translation_table=11, **kw)))


def _seeded_contigs():
    from metaeuk_amd import synth
    _, founders = synth.make_targets(300, 9)
    rs = np.random.RandomState(45)
    contigs = []
    for c in synth.make_contigs(25, founders, 9):
        s = np.array(list("ACGT"))[np.asarray(c)]
        for _ in range(max(1, len(s) // 400)):                       # N runs of 1 .. 30 over ~1.5 % of the bases
            p, n = rs.randint(len(s)), rs.randint(1, 31)
            s[p:p + n] = "N" if rs.rand() < 0.8 else "n"
        if rs.rand() < 0.5:                                          # a lower-case stretch
            p = rs.randint(len(s))
            s[p:p + 200] = [x.lower() for x in s[p:p + 200]]
        if rs.rand() < 0.3:
            s[rs.randint(len(s))] = "*"
        if rs.rand() < 0.5:                                          # codons that are '*' for the table and no stop for the scan
            for _ in range(20):
                p = rs.randint(len(s) - 3)
                s[p:p + 3] = list(rs.choice(["TAR", "UAA", "UGA", "TRA"]))
        contigs.append("".join(s))
    return contigs + ["AC", "", "NNNTAANNN", "ATG", "ATGTAA"], rs


def test_device_equals_the_twin_on_seeded_contigs(gpu_api):
    """synthetic contigs with N runs, lower case, junk and star codons: a dozen seeded combinations of code x start mode x all starts x
    contig start / end mode x gaps x frames x add-stop x reverse-fragments, device against host twin"""
    api = gpu_api
    contigs, rs = _seeded_contigs()
    seen, modes, stars = set(), set(), 0
    for i in range(14):
        mode = int(i % 3)
        kw = dict(translation_table=int(rs.choice(CODES)), orf_start_mode=mode, use_all_table_starts=int(rs.randint(0, 2)),
                  contig_start_mode=2 if mode == 1 else int(rs.choice([0, 1, 2, 2])), contig_end_mode=int(rs.choice([0, 1, 2, 2])),
                  min_codons=int(rs.choice([1, 5, 15, 40])), max_codons=int(rs.choice([100, 32734, 65533])),
                  max_gap_codons=int(rs.choice([0, 1, 2, 5, INT_MAX])), forward_frames=int(rs.randint(0, 8)), reverse_frames=int(rs.randint(0, 8)),
                  add_orf_stop=int(rs.randint(0, 2)), reverse_fragments=int(rs.randint(0, 2)))
        dev = api.Orfs(contigs, params=api.default_orf_params(**kw))
        _same_orfs(dev, api.Orfs(contigs, params=api.default_orf_params(**kw), host=True))
        seen.add(dev.n > 0)
        if dev.n:
            modes.add(mode)
            stars += kw["add_orf_stop"]
    assert True in seen and modes == {0, 1, 2} and stars > 0


def plain_q(api, db, orfs, params):
    q = orfs.queries(params)
    api.search(db, q)
    return q


def test_starred_orfs_feed_the_search(gpu_api):
    """--add-orf-stop: the codes the translate kernel wrote, stars included (X for the search), search like the same strings handed in as
    a query batch"""
    from metaeuk_amd import synth
    api = gpu_api
    targets, founders = synth.make_targets(300, 9)
    tstr = [synth.codes_to_str(t) for t in targets]
    contigs = ["".join("ACGT"[x] for x in c) for c in synth.make_contigs(25, founders, 9)]
    plain = api.Orfs(contigs)
    o = api.Orfs(contigs, params=api.default_orf_params(add_orf_stop=1))
    assert o.n == plain.n and int(o.aa_off[-1]) > int(plain.aa_off[-1])
    assert all(o.protein(k).strip("*") == plain.protein(k) for k in range(o.n)) and any(o.protein(k).count("*") == 2 for k in range(o.n))
    params = api.default_params()
    db = api.TargetDB(tstr, params)
    q1 = o.queries(params)                                       # (the results are views owned by the batch handles)
    (h1, ho1), (a1, ao1) = api.search(db, q1)
    q2 = api.Queries([o.protein(k) for k in range(o.n)], params)
    (h2, ho2), (a2, ao2) = api.search(db, q2)
    assert np.array_equal(np.asarray(ho1), np.asarray(ho2)) and h1.tobytes() == h2.tobytes()
    assert np.array_equal(np.asarray(ao1), np.asarray(ao2))
    n = int(ao1[-1])
    assert n > 20 and api.format_alignments(a1, 0, n) == api.format_alignments(a2, 0, n)
    # ... and stop there: exon coordinates are fragment start + 3 * query position, which an added leading star would shift
    with pytest.raises(api.MkError, match="add_orf_stop"):
        api.Predictions(db, o, q1)
    assert api.Predictions(db, plain, plain_q(api, db, plain, params)).n > 0


@pytest.mark.parametrize("tag,orf_kw", [("t6", dict(translation_table=6)), ("mode0", dict(orf_start_mode=0))])
def test_library_chain_equals_the_real_process(gpu_api, tag, orf_kw):
    """search_res and dp_predictions of the real binary's `predictexons -s 5.7 <flag>` on the e2e fixture, byte for byte, through the library:
    fragments -> query batch -> search -> exon sets (the fields belong to the library; the commands refuse the flags by name: tests/test_gpu_orf_flags.py)"""
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
    pred = api.Predictions(db, o, q)
    want = text("e2e_process_calls_%s.txt.gz" % tag)
    assert want.count("\t") > 500 and _prediction_text(pred, len(contigs)) == want
