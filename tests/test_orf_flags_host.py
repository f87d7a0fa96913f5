"""CPU test: the ORF-stage flags (--max-gaps, --forward-frames / --reverse-frames, --min-length / --max-length, --contig-end-mode,
--reverse-fragments) as the host twin mk_extract_orfs_host decides them -- the same restatement of the rule the kernels compile
(csrc/mk_orf_scan.hpp) -- against the output of the real `extractorfs` + `translatenucs` (tests/golden/PROVENANCE_orf_flags.txt)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_MAX = 2147483647

# case of tests/golden/make_orf_flag_golden.sh -> the flags it ran as mk_orf_params fields
CASES = {
    "maxgaps0": dict(max_gap_codons=0),
    "maxgaps2": dict(max_gap_codons=2),
    "fwd2_rev0": dict(forward_frames="2", reverse_frames="0"),
    "fwd13_rev2": dict(forward_frames="1,3", reverse_frames="2"),
    "len5_40": dict(min_codons=5, max_codons=40),
    "endmode0": dict(contig_end_mode=0),
    "endmode1": dict(contig_end_mode=1),
    "combo": dict(max_gap_codons=1, reverse_frames="3", contig_end_mode=1, max_codons=200),
}


def lines(name):
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        return f.read().split("\n")[:-1]


def text(name):
    with gzip.open(os.path.join(GOLD, name), "rt", encoding="latin-1") as f:
        return f.read()


def params_of(api, case):
    kw = dict(CASES[case])
    for k in ("forward_frames", "reverse_frames"):
        if k in kw:
            kw[k] = api.frame_mask(kw[k])
    return api.default_orf_params(**kw)


def orf_text(o, contig_count):
    """Orfs handle -> the block format of orf_expected.txt.gz: '>contig', then 'header<TAB>protein' per fragment"""
    out, k = [], 0
    for c in range(contig_count):
        out.append(">%d" % c)
        while k < o.n and int(o.orfs[k]["contig"]) == c:
            out.append(o.header(k) + "\t" + o.protein(k))
            k += 1
    assert k == o.n
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def api():
    from metaeuk_amd import api as a
    return a


@pytest.fixture(scope="module")
def flag_contigs():
    return lines("orf_flag_contigs.txt.gz")


def test_frame_mask_is_getframes(api):
    assert [api.frame_mask(s) for s in ("1,2,3", "1", "2", "3", "1,3", "0", "", "3,1,7", "12")] == [7, 1, 2, 4, 5, 0, 0, 5, 0]


def test_fixture_input_has_the_corners(flag_contigs):
    lens = [len(c) for c in flag_contigs]
    assert {2, 3, 5, 6} <= set(lens) and {n % 3 for n in lens} == {0, 1, 2} and max(lens) > 2 * 4096
    joined = "".join(flag_contigs)
    assert "n" in joined and "N" in joined and "*" in joined and "x" in joined


@pytest.mark.parametrize("case", sorted(CASES))
def test_twin_reproduces_the_reference(api, flag_contigs, case):
    o = api.Orfs(flag_contigs, params=params_of(api, case), host=True)
    exp = text("orf_flag_expected_%s.txt.gz" % case)
    assert o.n > 0 and o.n == exp.count("\n") - len(flag_contigs)
    assert orf_text(o, len(flag_contigs)) == exp


def test_twin_with_defaults_reproduces_the_existing_golden(api):
    contigs = lines("orf_contigs.txt.gz")
    exp = text("orf_expected.txt.gz")
    assert orf_text(api.Orfs(contigs, host=True), len(contigs)) == exp
    # an explicit "no limit" and the widest masks are the defaults
    p = api.default_orf_params(max_gap_codons=INT_MAX, forward_frames=7, reverse_frames=7, contig_end_mode=2)
    assert orf_text(api.Orfs(contigs, params=p, host=True), len(contigs)) == exp


def test_gap_limit_selects_by_gap_codons(api, flag_contigs):
    """--max-gaps G keeps exactly the default fragments with at most G gap codons, in the default order (a dropped fragment closes its frame)"""
    full = api.Orfs(flag_contigs, host=True)
    iupac = set("ACGTUMRWSYKVHDB")
    comp = dict(zip("ACGTUMRWSYKVHDBNacgtumrwsykvhdbn", "TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn"))

    def gaps(k):
        r = full.orfs[k]
        c = flag_contigs[int(r["contig"])]
        a, b = int(r["from"]), int(r["to"])
        nt = c[a:b + 1] if not r["minus_strand"] else "".join(comp.get("t" if x == "u" else x, "N") for x in c[b:a + 1][::-1])
        up = [chr(ord(x) & ~0x20) for x in nt]
        return sum(1 for i in range(0, len(up), 3) if any(x == "N" or x not in iupac for x in up[i:i + 3]))

    g = [gaps(k) for k in range(full.n)]
    assert {0, 1, 2, 3} <= set(g)
    for limit in (0, 1, 2, 3, 13):
        o = api.Orfs(flag_contigs, params=api.default_orf_params(max_gap_codons=limit), host=True)
        keep = [k for k in range(full.n) if g[k] <= limit]
        assert 0 < len(keep) < full.n
        assert [(o.header(i), o.protein(i)) for i in range(o.n)] == [(full.header(k), full.protein(k)) for k in keep]


def test_reversed_fragments_are_the_default_ones_back_to_front(api, flag_contigs):
    for kw in ({}, dict(max_gap_codons=1, reverse_frames=4, min_codons=5)):
        fwd = api.Orfs(flag_contigs, params=api.default_orf_params(**kw), host=True)
        rev = api.Orfs(flag_contigs, params=api.default_orf_params(reverse_fragments=1, **kw), host=True)
        assert rev.n == fwd.n > 0 and np.array_equal(rev.aa_off, fwd.aa_off) and rev.orfs.tobytes() == fwd.orfs.tobytes()
        assert [rev.header(k) for k in range(rev.n)] == [fwd.header(k) for k in range(fwd.n)]
        assert [rev.protein(k) for k in range(rev.n)] == [fwd.protein(k)[::-1] for k in range(fwd.n)]
        assert any(fwd.protein(k) != fwd.protein(k)[::-1] for k in range(fwd.n))


def test_reversed_fragments_equal_reverseseq_on_the_e2e_fixture(api):
    """the first 200 entries of the real aa_6f_reverse of `predictexons --reverse-fragments 1`"""
    contigs = lines("e2e_contigs.txt.gz")
    o = api.Orfs(contigs, params=api.default_orf_params(reverse_fragments=1), host=True)
    exp = text("e2e_process_aa_revfrag200.txt.gz")
    assert exp.count(">") == 200
    assert "".join(">%d\n%s\n" % (k, o.protein(k)) for k in range(200)) == exp


def test_disabled_strands_and_empty_answers(api, flag_contigs):
    full = api.Orfs(flag_contigs, host=True)
    plus = api.Orfs(flag_contigs, params=api.default_orf_params(reverse_frames=0), host=True)
    minus = api.Orfs(flag_contigs, params=api.default_orf_params(forward_frames=0), host=True)
    assert plus.n + minus.n == full.n and plus.n > 0 and minus.n > 0
    assert not plus.orfs["minus_strand"].any() and minus.orfs["minus_strand"].all()
    none = api.Orfs(flag_contigs, params=api.default_orf_params(forward_frames=0, reverse_frames=0), host=True)
    assert none.n == 0 and int(none.aa_off[-1]) == 0
    # the three single-frame runs of a strand partition it
    singles = [api.Orfs(flag_contigs, params=api.default_orf_params(forward_frames=0, reverse_frames=1 << f), host=True) for f in range(3)]
    assert sorted(h for o in singles for h in (o.header(k) for k in range(o.n))) == sorted(minus.header(k) for k in range(minus.n))
    assert api.Orfs([], host=True).n == 0 and api.Orfs(["", "AC"], host=True).n == 0


def test_argument_errors(api):
    raw, off, h = b"ACGTACGTAC", np.array([0, 10], dtype=np.uint64), C.c_void_p()

    def rc(**kw):
        p = api.default_orf_params(**kw)
        return api.lib().mk_extract_orfs_host(C.c_char_p(raw), off.ctypes.data_as(C.c_void_p), C.c_uint32(1), C.byref(p), C.byref(h))

    ARG, UNSUPPORTED = -1, -3
    assert rc() == 0
    api.lib().mk_orfs_destroy(h)
    for kw in (dict(forward_frames=8), dict(reverse_frames=8), dict(forward_frames=-1), dict(contig_end_mode=3), dict(contig_end_mode=-1),
               dict(max_codons=0), dict(min_codons=0), dict(max_gap_codons=-1), dict(reverse_fragments=2)):
        assert rc(**kw) == ARG, kw
    assert rc(max_codons=65535) == 0
    api.lib().mk_orfs_destroy(h)
    assert rc(max_codons=65536) == UNSUPPORTED and b"65535" in api.lib().mk_last_error()
    assert api.lib().mk_extract_orfs_host(C.c_char_p(raw), off.ctypes.data_as(C.c_void_p), C.c_uint32(1), None, C.byref(h)) == ARG
    with pytest.raises(TypeError):
        api.default_orf_params(max_gaps=1)
