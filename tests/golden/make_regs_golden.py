"""Writes tests/golden/regs_kat.json: known answers of mm_set_parent + mm_select_sub for tables of two or three regions, worked out on paper
below - neither the oracle nor the model of tests/regs_ref.py is asked.  Run from the repository root: python tests/golden/make_regs_golden.py

A region is (score, cnt, qs, qe, rs, re, rev, rid, inv); regions stand in mm_gen_regs' order.  An answer row is (row in the table, parent,
subsc, n_sub, strand_retained) per region kept, parent being the parent's place among the kept ones.  Unless said otherwise: mask_level 0.5,
pri_ratio 0.5, min_diff 42 (2 k, k = 21), best_n 20, min_strand_sc 80.  Every region has 3 anchors, so a secondary always counts in n_sub.

at-level     A = [0, 100), B = [25, 125).  They share 75 bases of min(100, 100); 25 bases of B lie outside A, of max(100, 100):
             75/100 - 25/100 = 0.5 (0.75 and 0.25 are exact in binary), which is not ABOVE 0.5: B is a primary of its own.
above        B = [24, 124): 76/100 - 24/100 = 0.52 > 0.5: B's parent is A; A.subsc = B's score 900, A.n_sub = 1.  900 >= 1000 * 0.5: kept.
ratio-drop   B = [10, 90) inside A (80/80 - 0 = 1 > 0.5), score 499 < 1000 * 0.5 and 499 + 42 < 1000; same strand: dropped.  A keeps
             subsc 499 and n_sub 1 from set_parent.
ratio-0.8    pri_ratio 0.8, B's score 800.  0.8 is not a binary fraction: as float32 it is 0.800000011920929, times 1000 = 800.0000119, which
             rounds to the float32 800.0 (its neighbours are 6.1e-5 away): 800 >= 800.0 holds and B is kept.  (In double 800 < 800.0000119.)
strand       A = [0, 300) forward at 1000..1300 of contig 0; B = [100, 200) on the reverse strand at 1120..1220, score 90.  B lies inside A
             (parent A).  90 < 500 and 90 + 42 < 1000, but 90 > 80, the strands differ, the contig is the same and 1120 < 1300, 1220 > 1000:
             kept with strand_retained = 1.
drop-sync    A = [0, 100) 1000, B = [10, 90) 400 (child of A, dropped: 400 < 500, 442 < 1000), C = [200, 300) 300, a primary.  C moves to
             place 1; mm_sync_regs renumbers it: id 1, parent 1.
same-coords  best_n = 1.  B has A's coordinates and score 900: within the ratio, but a secondary with its parent's exact coordinates is dropped
             WITHOUT being counted; C = [10, 90) 800 is therefore still the first secondary and is kept.  A.subsc = 900, A.n_sub = 2.
touch        A = [0, 100), B = [100, 200): A ends where B starts, which is no overlap: both primaries.
"""
import json
import os

R0 = 1000


def r(score, qs, qe, rev=0, rs=None, re=None):
    return [score, 3, qs, qe, R0 + qs if rs is None else rs, R0 + qe if re is None else re, rev, 0, 0]


PAR = dict(mask_level=0.5, pri_ratio=0.5, min_diff=42, best_n=20, min_strand_sc=80)
CASES = [
    dict(name="at-level", tab=[r(1000, 0, 100), r(900, 25, 125)], rows=[[0, 0, 0, 0, 0], [1, 1, 0, 0, 0]]),
    dict(name="above", tab=[r(1000, 0, 100), r(900, 24, 124)], rows=[[0, 0, 900, 1, 0], [1, 0, 0, 0, 0]]),
    dict(name="ratio-drop", tab=[r(1000, 0, 100), r(499, 10, 90)], rows=[[0, 0, 499, 1, 0]]),
    dict(name="ratio-0.8", par=dict(pri_ratio=0.8), tab=[r(1000, 0, 100), r(800, 10, 90)], rows=[[0, 0, 800, 1, 0], [1, 0, 0, 0, 0]]),
    dict(name="strand", tab=[r(1000, 0, 300), r(90, 100, 200, rev=1, rs=R0 + 120, re=R0 + 220)], rows=[[0, 0, 90, 1, 0], [1, 0, 0, 0, 1]]),
    dict(name="drop-sync", tab=[r(1000, 0, 100), r(400, 10, 90), r(300, 200, 300)], rows=[[0, 0, 400, 1, 0], [2, 1, 0, 0, 0]]),
    dict(name="same-coords", par=dict(best_n=1), tab=[r(1000, 0, 100), r(900, 0, 100), r(800, 10, 90)], rows=[[0, 0, 900, 2, 0], [2, 0, 0, 0, 0]]),
    dict(name="touch", tab=[r(1000, 0, 100), r(900, 100, 200)], rows=[[0, 0, 0, 0, 0], [1, 1, 0, 0, 0]]),
]

if __name__ == "__main__":
    out = dict(columns=dict(tab=["score", "cnt", "qs", "qe", "rs", "re", "rev", "rid", "inv"], rows=["row", "parent", "subsc", "n_sub", "strand_retained"]),
               cases=[dict(name=c["name"], par=dict(PAR, **c.get("par", {})), tab=c["tab"], rows=c["rows"]) for c in CASES])
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "regs_kat.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
