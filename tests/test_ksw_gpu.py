"""The two device alignment kernels, called directly (sh_dbg_ksw_extd2 / sh_dbg_ksw_ll, csrc/sh_dbg_align.hip) on the case table of
tests/ksw_cases.py: ksw_extd2_core through both dispatches the product has, in all three storage forms and both cell loops, and
lr_ksw_ll_wave, bit for bit against the oracle's mma_ksw_extd2 / mma_ksw_ll and - for the known-answer sets - against the plain
dynamic programme's numbers.  Integers only: there is no tolerance anywhere."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import ksw_cases as K

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


class KswCase(C.Structure):
    _fields_ = [("q_off", C.c_uint64), ("t_off", C.c_uint64)] + [(n, C.c_int32) for n in
                ("qlen", "tlen", "a", "b", "sc_ambi", "q", "e", "q2", "e2", "w", "zdrop", "end_bonus", "flag", "route", "unsized", "pad")]


class KswResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in K.EZ_FIELDS + ("form",)] + [("cigar_off", C.c_uint64)]


class LlCase(C.Structure):
    _fields_ = [("q_off", C.c_uint64), ("t_off", C.c_uint64)] + [(n, C.c_int32) for n in ("qlen", "tlen", "a", "b", "sc_ambi", "gapo", "gape", "pad")]


class LlResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("score", "qe", "te", "pad")]


def _blob(seqs, shift):
    """every sequence at `shift` bytes past a multiple of 8 (shift None: back to back, so at whatever offset the lengths leave)"""
    offs, parts, pos = [], [], 0
    for s in seqs:
        if shift is not None:
            pad = (shift - pos) % 8
            parts.append(np.full(pad, 4, np.uint8)); pos += pad
        offs.append(pos); parts.append(np.ascontiguousarray(s, np.uint8)); pos += len(s)
    return np.concatenate(parts + [np.full(8, 4, np.uint8)]), offs


def run_extd2(entries, shift=0):
    """entries: (case, route, unsized).  One launch; returns [({field: value}, [cigar words], form)]."""
    from scrubby_amd import lib as S
    L = S.require_gpu()
    blob, offs = _blob([x for c, _, _ in entries for x in (c["query"], c["target"])], shift)
    arr = (KswCase * len(entries))()
    for i, (c, route, unsized) in enumerate(entries):
        k = arr[i]
        k.q_off, k.t_off, k.qlen, k.tlen = offs[2 * i], offs[2 * i + 1], len(c["query"]), len(c["target"])
        for f in ("a", "b", "sc_ambi", "q", "e", "q2", "e2", "w", "zdrop", "end_bonus", "flag"):
            setattr(k, f, c[f])
        k.route, k.unsized = route, int(unsized)
    out = (KswResult * len(entries))()
    n_words = sum(len(c["query"]) + len(c["target"]) for c, _, _ in entries)
    cig = np.zeros(n_words, np.uint32)
    S.check(L.sh_dbg_ksw_extd2(0, blob.ctypes.data, len(blob), C.cast(arr, C.c_void_p), len(entries), C.cast(out, C.c_void_p), cig.ctypes.data, n_words))
    res = []
    for r in out:
        assert 0 <= r.n_cigar and r.cigar_off + r.n_cigar <= n_words
        res.append(({f: int(getattr(r, f)) for f in K.EZ_FIELDS}, [int(x) for x in cig[r.cigar_off:r.cigar_off + r.n_cigar]], int(r.form)))
    return res


@pytest.fixture(scope="module")
def entries():
    return [(c, route, False) for c in K.extd2_table() for route in c["routes"]]


@pytest.fixture(scope="module")
def want(oracle):
    L = oracle.lib()
    return {c["name"]: K.oracle_extd2(L, c) for c in K.extd2_table()}


@pytest.fixture(scope="module")
def device(entries):
    """the whole table on every route it applies to, in one launch, every sequence on a multiple of 8 bytes"""
    return run_extd2(entries, 0)


def _differences(entries, got, want):
    bad = []
    for (c, route, _), (ez, cig, _) in zip(entries, got):
        wez, wcig = want[c["name"]]
        if ez != wez or cig != wcig:
            bad.append((c["name"], route, {f: (ez[f], wez[f]) for f in K.EZ_FIELDS if ez[f] != wez[f]}, "cigar differs" if cig != wcig else ""))
    return bad


@pytest.mark.parametrize("route", [0, 1])
def test_every_case_is_bit_identical_to_the_oracle(entries, device, want, route):
    """all eleven fields of ksw_extz_t and the CIGAR; route 0 = the short-read dispatch (three storage forms), 1 = the long-read one"""
    sel = [i for i, e in enumerate(entries) if e[1] == route]
    assert len(sel) >= 400
    bad = _differences([entries[i] for i in sel], [device[i] for i in sel], want)
    assert not bad, (len(bad), bad[:8])


def test_the_dispatch_takes_the_form_the_table_predicts(entries, device):
    seen = set()
    for (c, route, _), (_, _, form) in zip(entries, device):
        assert form == K.form(route, len(c["query"]), len(c["target"]), c["w"]), (c["name"], route, form)
        seen.add((route, form))
    assert seen == {(0, 0), (0, 1), (0, 2), (1, 1), (1, 2)}


@pytest.mark.parametrize("shift", [1, 2, 3, 4, 5, 6, 7])
def test_results_do_not_depend_on_where_a_sequence_starts(entries, device, shift):
    got = run_extd2(entries, shift)
    bad = [(e[0]["name"], e[1]) for e, g, d in zip(entries, got, device) if g != d]
    assert not bad, (len(bad), bad[:8])


def test_known_answers_on_the_device():
    """score / max / mqe / mte of the plain dynamic programme (tests/golden/make_align_golden.py), small and wide sets, asserted on the
    device's results directly: the oracle is not in this test."""
    from tests.test_align_oracle_cpu import kat_wide
    small = json.load(open(os.path.join(HERE, "golden", "align_kat.json")))["cases"]
    wide = kat_wide()
    assert len(small) >= 100 and len(wide) >= 24
    ent = []
    for cases, w, routes in ((small, 200, (0,)), (wide, -1, (0, 1))):
        for c in cases:
            for flag in (0, 0x40, 0x40 | 0x02 | 0x80, 0x02):
                for route in routes:
                    ent.append((dict(c, w=w, zdrop=-1, end_bonus=10 if flag & 0x40 else -1, flag=flag), route, False))
    got = run_extd2(ent, None)
    bad = []
    for (c, route, _), (ez, cig, form) in zip(ent, got):
        x = c["expect"]
        if (ez["score"], ez["max"], ez["mqe"], ez["mte"]) != (x["score"], x["max"], x["mqe"], x["mte"]) or ez["zdropped"] or (not cig and not c["flag"] & 0x40):
            bad.append((len(c["query"]), len(c["target"]), c["flag"], route, form, ez, x))
    assert not bad, (len(bad), bad[:5])
    assert {form for _, _, form in got} == {0, 1, 2}


def test_a_case_beyond_its_scratch_is_given_up_and_its_neighbours_are_not(oracle):
    from scrubby_amd import lib as S
    L = oracle.lib()
    mk = lambda ql, tl, w, flag, seed: K._case(f"scratch:{ql}x{tl}w{w}", "related", ql, tl, w, seed % 3, flag, -1, 10 if flag & 0x40 else -1, (0, 1), seed)
    small_a, small_b, small_c, banded = mk(100, 100, -1, 0x40, 1), mk(128, 128, -1, 0, 2), mk(64, 65, 5, 0, 3), mk(400, 400, 3, 0x40, 4)
    # 599 rows of 320 direction bytes: its bases fit the scratch the 400 x 400 band asks for, its direction bytes are five times what
    # 128 x 128 asks for
    big = mk(300, 300, -1, 0x40, 5)
    ent = [(small_a, 0, False), (big, 0, True), (small_b, 0, False), (small_c, 0, False), (big, 1, True), (small_b, 1, False), (banded, 0, False)]
    got = run_extd2(ent, 3)
    reset = {"max": 0, "zdropped": 0, "max_q": -1, "max_t": -1, "mqe": -0x40000000, "mqe_t": -1, "mte": -0x40000000, "mte_q": -1, "score": -0x40000000, "reach_end": 0, "n_cigar": 0}
    assert got[1] == (dict(reset, zdropped=1), [], 1)      # ksw_extd2_core: "outside the context's sizing"
    assert got[4] == (reset, [], -1)                        # lr_align_pair: the read goes to the large-scratch pass, nothing ran
    for i in (0, 2, 3, 5, 6):
        wez, wcig = K.oracle_extd2(L, ent[i][0])
        assert got[i][:2] == (wez, wcig), ent[i][0]["name"]
    assert [g[2] for g in got] == [1, 1, 1, 0, -1, 1, 2]
    with pytest.raises(S.ScrubbyHipError):      # an unsized case that would fit is refused before anything is launched
        run_extd2([(big, 0, False), (small_a, 0, True)], 0)


def test_local_alignment_is_identical_to_the_oracle(oracle):
    from scrubby_amd import lib as S
    G = S.require_gpu()
    L = oracle.lib()
    table = K.ll_table()
    blob, offs = _blob([x for c in table for x in (c["query"], c["target"])], None)
    assert {o % 8 for o in offs} == set(range(8))
    arr = (LlCase * len(table))()
    for i, c in enumerate(table):
        k = arr[i]
        k.q_off, k.t_off, k.qlen, k.tlen = offs[2 * i], offs[2 * i + 1], len(c["query"]), len(c["target"])
        for f in ("a", "b", "sc_ambi", "gapo", "gape"):
            setattr(k, f, c[f])
    out = (LlResult * len(table))()
    S.check(G.sh_dbg_ksw_ll(0, blob.ctypes.data, len(blob), C.cast(arr, C.c_void_p), len(table), C.cast(out, C.c_void_p)))
    bad = []
    for c, r in zip(table, out):
        w = K.oracle_ll(L, c)
        if (r.score, r.qe, r.te) != w:
            bad.append((c["name"], (r.score, r.qe, r.te), w))
    assert not bad, (len(bad), bad[:8])
