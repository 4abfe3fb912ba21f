"""The case table of the device alignment kernels (tests/ksw_cases.py) reaches what it is meant to reach: every storage form with every
cell loop that can exist, both sides of every border, z-drops that fire and that do not, maxima that tie.  Checked on the CPU, against
the oracle and the plain dynamic programme, so that a GPU visit is not spent on a table with a hole in it."""
import importlib.util
import os

import numpy as np

from tests import ksw_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))


def _shape(c):
    return len(c["query"]), len(c["target"]), c["w"]


def test_every_storage_form_meets_every_cell_loop_that_can_exist():
    """Form 0 holds at most AL_P = 4096 direction bytes, (qlen + tlen - 1) rows of n_col >= min(qlen, tlen, w + 1) + 16 each.  A rounded
    range of more than 64 cells takes a band of at least 50, so n_col >= 80 and at most 51 rows - but a band of 50 cells needs at least
    99 anti-diagonals' worth of bases.  So form 0 never sees a second step of the narrow loop and never the wide loop; the forms with
    the directions in HBM see all four."""
    seen = {}
    for c in K.extd2_table():
        ql, tl, w = _shape(c)
        for route in c["routes"]:
            key = (K.form(route, ql, tl, w),) + tuple(min(x, 2) if isinstance(x, int) else x for x in K.loop_class(ql, tl, w))
            seen[key] = seen.get(key, 0) + 1
    for f in (0, 1, 2):
        for loop in ("narrow", "wide"):
            for steps in (1, 2):
                if f == 0 and (loop, steps) != ("narrow", 1):
                    assert (f, loop, steps) not in seen
                else:
                    assert seen.get((f, loop, steps), 0) >= 2, (f, loop, steps, seen)
    for ql in range(1, 340, 7):      # the impossibility claimed above, over a grid of shapes rather than by argument alone
        for tl in range(1, 460, 9):
            for w in (-1, 3, 20, 50, 64, 100):
                if K.form(0, ql, tl, w) == 0:
                    assert K.loop_class(ql, tl, w) == ("narrow", 1)


def test_both_sides_of_every_border_are_in_the_table():
    table = K.extd2_table()
    shapes = {_shape(c) for c in table}
    widths = {K.widest(*s) for s in shapes}
    for lo, hi in ((64, 80), (128, 144), (256, 272)):      # rounded ranges come in multiples of 16
        assert lo in widths and hi in widths, (lo, hi, sorted(widths))
    for n in K.SQUARES:
        assert (n, n, -1) in shapes
    for w in K.BANDS_400:
        assert (400, 400, w) in shapes
    # the band of 400 x 400 puts w and w + 1 cells on alternate diagonals, rounded to 16 from wherever they start: w = 127 runs diagonals of
    # 128 cells through the narrow loop and of 144 through the wide one, w = 255 one and two steps of the wide loop
    for w, lo, hi in ((127, 128, 144), (255, 256, 272)):
        assert {lo, hi} <= {en - st + 1 for _, _, st, en in K.ranges(400, 400, w)}
    assert [K.loop_class(400, 400, w) for w in (127, 128, 129)] == [("wide", 1)] * 3
    assert K.loop_class(400, 400, 3) == ("narrow", 1)
    assert [K.loop_class(400, 400, w) for w in (255, 256, 257)] == [("wide", 2)] * 3
    for q, t in K.UNEQUAL:
        assert (q, t, -1) in shapes
    # direction bytes around AL_P, on the route that can keep them in LDS
    assert K.p_need(32, 32, -1) == 3024 and K.p_need(33, 33, -1) == 4160 and K.form(0, 32, 32, -1) == 0 and K.form(0, 33, 33, -1) == 1
    assert K.p_need(64, 65, 5) <= K.AL_P < K.p_need(65, 65, 5) and K.form(0, 64, 65, 5) == 0 and K.form(0, 65, 65, 5) == 1
    # the state around AL_T16 and AL_Q16, on both routes
    for route in (0, 1):
        assert [K.form(route, q, t, -1) for q, t in K.STATE_BORDER] == [1, 2, 1, 2]
    for s in K.P_BORDER + [(q, t, -1) for q, t in K.STATE_BORDER]:
        assert s in shapes
    assert K.BIG in shapes and all(c["routes"] == (1,) for c in table if _shape(c) == K.BIG)
    # every shape runs as a global alignment and as an extension; every flag meets every form and both loops
    for s in K.shapes():
        assert {0, 0x40} <= {c["flag"] for c in table if _shape(c) == s}, s
    for flag in K.FLAGS:
        met = set()
        for c in table:
            if c["flag"] == flag:
                for route in c["routes"]:
                    met.add((K.form(route, *_shape(c)), K.loop_class(*_shape(c))[0]))
        assert met >= {(0, "narrow"), (1, "narrow"), (1, "wide"), (2, "narrow"), (2, "wide")}, (flag, met)
    assert {c["zdrop"] for c in table} >= {-1, 100, 400} and {c["end_bonus"] for c in table} >= {-1, 10}
    assert {(c["a"], c["b"], c["sc_ambi"], c["q"], c["e"], c["q2"], c["e2"]) for c in table} == set(K.SCORES)
    assert any((c["query"] == 4).any() or (c["target"] == 4).any() for c in table)
    assert len({c["name"] for c in table}) == len(table)
    # the local alignment: every padding of the query (qlen % 8), the chunk carry of F (more than 64 padded columns), every target length
    ll = {(len(c["query"]), len(c["target"])) for c in K.ll_table()}
    assert ll == {(q, t) for q in K.LL_QLEN for t in K.LL_TLEN}
    assert {q % 8 for q in K.LL_QLEN} >= {0, 1, 7} and {((q + 7) // 8 * 8 - 1) // 64 for q in K.LL_QLEN} >= {0, 1, 7, 8}


def test_the_table_is_deterministic():
    a, b = K.extd2_cases(), K.extd2_cases()
    assert all(x["name"] == y["name"] and np.array_equal(x["query"], y["query"]) and np.array_equal(x["target"], y["target"]) for x, y in zip(a, b))


def test_zdrop_fires_and_does_not(oracle):
    L = oracle.lib()
    z = [K.oracle_extd2(L, c)[0]["zdropped"] for c in K.extd2_table() if c["family"] == "zdrop"]
    assert z.count(1) >= 5 and z.count(0) >= 5, (z.count(1), z.count(0))


def test_maxima_tie(oracle):
    """At least ten cases hold their final maximum in more than one cell of the matrix (the plain dynamic programme of
    tests/golden/make_align_golden.py says where), and the local alignment's best row holds its maximum in more than one column in at
    least ten cases: the places where the order in which the kernels scan matters."""
    spec = importlib.util.spec_from_file_location("make_align_golden", os.path.join(HERE, "golden", "make_align_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    L = oracle.lib()
    tied = 0
    for c in K.extd2_table():
        ql, tl, w = _shape(c)
        if c["family"] != "ties" or ql * tl > 100000 or (w >= 0 and w < max(ql, tl)):
            continue
        H = G.plain_matrix(list(c["query"]), list(c["target"]), c["a"], c["b"], c["sc_ambi"], c["q"], c["e"], c["q2"], c["e2"])
        ez, _ = K.oracle_extd2(L, c)
        if H.max() > 0 and ez["max"] == int(H.max()) and int((H == H.max()).sum()) > 1:
            tied += 1
    assert tied >= 10, tied
    tied_ll = 0
    for c in K.ll_table():
        sc, qe, te = K.oracle_ll(L, c)
        q, t = c["query"], c["target"]
        if sc > 0 and te > 0:      # rows before te that reach the same score: the LAST one must win
            s2, _, te2 = K.oracle_ll(L, dict(c, target=t[:te]))
            tied_ll += s2 == sc
    assert tied_ll >= 10, tied_ll
