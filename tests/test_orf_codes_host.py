"""CPU test: the genetic code (--translation-table), the ORF start modes (--orf-start-mode, --use-all-table-starts, --contig-start-mode)
and --add-orf-stop as the host twin mk_extract_orfs_host decides them -- the same restatement of the rule the kernels compile
(csrc/mk_orf_scan.hpp) -- against the output of the real `extractorfs` + `translatenucs` (tests/golden/PROVENANCE_orf_codes.txt)."""
import ctypes as C

import numpy as np
import pytest

from test_orf_flags_host import CASES as FLAG_CASES, lines, orf_text, params_of as flag_params_of, text

CODES = (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31)     # TranslateNucl::GenCode

# case of tests/golden/make_orf_code_golden.sh -> the flags it ran as mk_orf_params fields
CASES = {
    "t6": dict(translation_table=6),
    "t2": dict(translation_table=2),
    "t22": dict(translation_table=22),
    "mode0": dict(orf_start_mode=0),
    "mode2": dict(orf_start_mode=2),
    "mode0_cs1": dict(orf_start_mode=0, contig_start_mode=1),
    "mode2_cs0": dict(orf_start_mode=2, contig_start_mode=0),
    "mode0_gaps1": dict(orf_start_mode=0, max_gap_codons=1),
    "mode2_gaps1": dict(orf_start_mode=2, max_gap_codons=1),
    "t4_mode0_all": dict(translation_table=4, orf_start_mode=0, use_all_table_starts=1),
    "t11_mode2_all_combo": dict(translation_table=11, orf_start_mode=2, use_all_table_starts=1, reverse_frames="2", contig_end_mode=1),
    "addstop": dict(add_orf_stop=1),
    "addstop_mode0_t6": dict(add_orf_stop=1, orf_start_mode=0, translation_table=6),
}


def params_of(api, case):
    kw = dict(CASES[case])
    for k in ("forward_frames", "reverse_frames"):
        if k in kw:
            kw[k] = api.frame_mask(kw[k])
    return api.default_orf_params(**kw)


def all_codons():
    a = "ACMGRSVTWYHKDBN"
    return "".join(x + y + z for x in a for y in a for z in a)


@pytest.fixture(scope="module")
def api():
    from metaeuk_amd import api as a
    return a


@pytest.fixture(scope="module")
def code_contigs():
    return lines("orf_code_contigs.txt.gz")


def test_defaults_of_the_new_fields(api):
    p = api.default_orf_params()
    assert (p.translation_table, p.orf_start_mode, p.use_all_table_starts, p.contig_start_mode, p.add_orf_stop) == (1, 1, 0, 2, 0)


def test_fixture_input_has_the_corners(code_contigs):
    lens = [len(c) for c in code_contigs]
    assert {2, 3, 5, 6, 4099} <= set(lens) and {n % 3 for n in lens} == {0, 1, 2} and max(lens) > 2 * 4096 and len(lens) < 64
    joined = "".join(code_contigs)
    for s in ("UAATAA", "TARTGA", "uaataa", "taa", "atg", "aTG", "N" * 40, "ATGTAA"):
        assert s in joined, s


@pytest.mark.parametrize("case", sorted(CASES))
def test_twin_reproduces_the_reference(api, code_contigs, case):
    o = api.Orfs(code_contigs, params=params_of(api, case), host=True)
    exp = text("orf_code_expected_%s.txt.gz" % case)
    assert o.n > 0 and o.n == exp.count("\n") - len(code_contigs)
    assert orf_text(o, len(code_contigs)) == exp


def test_twin_translates_every_codon_under_every_code(api):
    """all 15^3 IUPAC codons through the real `translatenucs --translation-table T`: the whole table of each of the 25 codes.  The twin
    translates fragments, so the entry is scanned in forward frame 1 without a length limit: the fragments cover every codon but the
    stops of the code, and those are '*' by definition -- which also ties the stop set of the scan to the table"""
    codons = all_codons()
    rows = dict(l.split("\t") for l in lines("orf_code_tables.txt.gz"))
    assert sorted(map(int, rows)) == list(CODES) and len(set(rows.values())) > 20
    for t in CODES:
        want = rows[str(t)]
        assert len(want) == 15 ** 3
        o = api.Orfs([codons], params=api.default_orf_params(translation_table=t, min_codons=1, forward_frames=1, reverse_frames=0), host=True)
        got = ["*"] * (15 ** 3)                                     # a codon no fragment covers closed one: a stop of the code
        for k in range(o.n):
            a = int(o.orfs[k]["from"]) // 3
            got[a:a + len(o.protein(k))] = o.protein(k)
        assert "".join(got) == want, t
        assert want.count("*") >= o.n - 1                           # (TAR and its like translate to '*' inside a fragment; codes 27, 28, 31 have no stop)


def starts_params(api, t):
    return api.default_orf_params(translation_table=t, orf_start_mode=2, use_all_table_starts=1)


def test_twin_has_the_start_set_of_every_code(api, code_contigs):
    """the headers of the real `extractorfs --orf-start-mode 2 --use-all-table-starts 1 --translation-table T` for all 25 codes: mode 2 moves a
    fragment's begin to every start codon, so one wrong member of a start (or stop) set moves a header"""
    blocks = text("orf_code_starts.txt.gz").split("#")[1:]
    assert [int(b.split("\n", 1)[0]) for b in blocks] == list(CODES) and len({b.split("\n", 1)[1] for b in blocks}) >= 18
    for b in blocks:
        t, want = b.split("\n", 1)
        o = api.Orfs(code_contigs, params=starts_params(api, int(t)), host=True)
        assert o.n > 100 and "".join(o.header(k) + "\n" for k in range(o.n)) == want, t


def test_defaults_still_give_the_existing_goldens(api):
    contigs = lines("orf_contigs.txt.gz")
    assert orf_text(api.Orfs(contigs, host=True), len(contigs)) == text("orf_expected.txt.gz")
    flag_contigs = lines("orf_flag_contigs.txt.gz")
    for case in sorted(FLAG_CASES):
        o = api.Orfs(flag_contigs, params=flag_params_of(api, case), host=True)
        assert orf_text(o, len(flag_contigs)) == text("orf_flag_expected_%s.txt.gz" % case), case


def test_general_walk_equals_the_default_walk_where_the_rules_coincide(api, code_contigs):
    """genetic code 11 has the stops and the residues of code 1, so with start mode 1 the walk over the stop set must give what the
    spelled-out default walk gives -- with and without a gap limit, on both fixture inputs"""
    for contigs in (code_contigs, lines("orf_flag_contigs.txt.gz")):
        for kw in ({}, dict(max_gap_codons=0), dict(max_gap_codons=2, contig_end_mode=1, min_codons=1), dict(forward_frames=5, reverse_frames=2, max_codons=40)):
            a = api.Orfs(contigs, params=api.default_orf_params(**kw), host=True)
            b = api.Orfs(contigs, params=api.default_orf_params(translation_table=11, **kw), host=True)
            assert a.n == b.n > 0 and a.orfs.tobytes() == b.orfs.tobytes() and a.aa == b.aa and np.array_equal(a.aa_off, b.aa_off)


def test_all_table_starts_have_no_effect_in_mode_1(api, code_contigs):
    a = api.Orfs(code_contigs, params=api.default_orf_params(translation_table=4), host=True)
    b = api.Orfs(code_contigs, params=api.default_orf_params(translation_table=4, use_all_table_starts=1), host=True)
    assert a.n == b.n > 0 and a.orfs.tobytes() == b.orfs.tobytes() and a.aa == b.aa


def test_stars_mirror_with_the_fragment(api, code_contigs):
    """--reverse-fragments after --add-orf-stop: reverseseq runs on translatenucs' output, so the stars change ends with the residues"""
    for kw in (dict(add_orf_stop=1), dict(add_orf_stop=1, orf_start_mode=2, translation_table=6, max_gap_codons=1)):
        fwd = api.Orfs(code_contigs, params=api.default_orf_params(**kw), host=True)
        rev = api.Orfs(code_contigs, params=api.default_orf_params(reverse_fragments=1, **kw), host=True)
        assert rev.n == fwd.n > 0 and np.array_equal(rev.aa_off, fwd.aa_off) and rev.orfs.tobytes() == fwd.orfs.tobytes()
        assert [rev.protein(k) for k in range(rev.n)] == [fwd.protein(k)[::-1] for k in range(fwd.n)]
        stars = {(fwd.protein(k)[0] == "*", fwd.protein(k)[-1] == "*") for k in range(fwd.n)}
        assert {(True, True), (True, False), (False, True)} <= stars


def test_argument_errors(api):
    raw, off, h = b"ACGTACGTAC", np.array([0, 10], dtype=np.uint64), C.c_void_p()

    def rc(**kw):
        p = api.default_orf_params(**kw)
        r = api.lib().mk_extract_orfs_host(C.c_char_p(raw), off.ctypes.data_as(C.c_void_p), C.c_uint32(1), C.byref(p), C.byref(h))
        if r == 0:
            api.lib().mk_orfs_destroy(h)
        return r

    ARG, UNSUPPORTED = -1, -3
    for t in CODES:
        assert rc(translation_table=t) == 0, t
    for t in (0, 7, 8, 17, 20, 32, -1):
        assert rc(translation_table=t) == ARG, t
    assert b"translation_table" in api.lib().mk_last_error()
    for kw in (dict(orf_start_mode=3), dict(orf_start_mode=-1), dict(orf_start_mode=1, contig_start_mode=0), dict(orf_start_mode=1, contig_start_mode=1),
               dict(contig_start_mode=0), dict(orf_start_mode=0, contig_start_mode=3), dict(use_all_table_starts=2), dict(use_all_table_starts=-1),
               dict(add_orf_stop=2), dict(add_orf_stop=-1)):
        assert rc(**kw) == ARG, kw
    for kw in (dict(orf_start_mode=0, contig_start_mode=0), dict(orf_start_mode=2, contig_start_mode=1), dict(orf_start_mode=0, use_all_table_starts=1),
               dict(add_orf_stop=1, max_codons=65533), dict(max_codons=65534)):
        assert rc(**kw) == 0, kw
    assert rc(add_orf_stop=1, max_codons=65534) == UNSUPPORTED and b"65533" in api.lib().mk_last_error()
