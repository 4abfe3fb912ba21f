"""A plain model of the region bookkeeping between "a read's chains" and the base-level alignment: the order mm_gen_regs gives, mm_set_parent,
mm_select_sub and mm_sync_regs, written from the definitions in minimap2's hit.c as DESIGN.md / SURVEY.md App. A.6 recall them - not from
oracle/mm_align.c, whose statements it does not follow.  Integers are Python integers; the three float steps (the two quotients against
mask_level, the product against pri_ratio) are numpy.float32 in the operation order of the C.

A region is a dict with score, cnt, qs, qe, rs, re, rev, rid, inv (inputs) and id, parent, subsc, n_sub, strand_retained (results)."""
import numpy as np

M64, M32 = (1 << 64) - 1, (1 << 32) - 1
UNSET = -1
F = np.float32


def hash64(key):
    """Thomas Wang's 64-bit mix, as minimap2 uses it without a mask"""
    key = (~key + (key << 21)) & M64
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & M64
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & M64
    key ^= key >> 28
    return (key + (key << 31)) & M64


def wang32(key):
    key = (key + (~(key << 15) & M32)) & M32
    key ^= key >> 10
    key = (key + (key << 3)) & M32
    key ^= key >> 6
    key = (key + (~(key << 11) & M32)) & M32
    return key ^ key >> 16


def read_hash(qlen, seed=11):
    """mm_map_frag: the hash of a read without a name - its length and opt->seed"""
    return wang32((wang32(qlen) + wang32(seed)) & M32)


def chain_key(x0, y0, score, cnt, rhash):
    """the sort key of a chain whose first anchor is (x0, y0): (score << 32 | cnt) with the low word scrambled by the anchor"""
    h = hash64(((hash64(x0) + hash64(y0)) & M64) ^ rhash) & M32
    return ((score & M32) << 32 | cnt) ^ h


def gen_order(keys):
    """the order of the regions: key descending; among equal keys the chain that stands LATER in u[] comes first (a stable ascending sort,
    reversed).  keys[i] belongs to chain i of u[]; returns the chain indices."""
    return sorted(range(len(keys)), key=lambda i: (-keys[i], -i))


def anchor_coords(xs, qs, k, qlen):
    """qs, qe, rs, re, rev, rid of a chain with anchors (x = strand << 63 | rid << 32 | last ref base, q = last query base on that strand)"""
    rev, rid = xs[0] >> 63, (xs[0] & ((1 << 63) - 1)) >> 32
    r0, r1 = xs[0] & M32, xs[-1] & M32
    out = dict(rev=int(rev), rid=int(rid), rs=max(int(r0) + 1 - k, 0), re=int(r1) + 1)
    if rev:
        out.update(qs=qlen - (int(qs[-1]) + 1), qe=qlen - (int(qs[0]) + 1 - k))
    else:
        out.update(qs=int(qs[0]) + 1 - k, qe=int(qs[-1]) + 1)
    return out


def _union_len(ivs):
    """total length of a union of half-open intervals"""
    n, end = 0, None
    for s, e in sorted(ivs):
        if end is None or s > end:
            n += e - s
            end = e
        elif e > end:
            n += e - end
            end = e
    return n


def set_parent(regs, mask_level):
    """Walk the regions in order.  Against the primaries found so far that overlap region i on the query: the part of i none of them covers
    (uncov), and for each of them in the order they became primary ol / min(len) - uncov / max(len); the first above mask_level becomes i's
    parent, takes i's score into subsc and counts i in n_sub when i has at least as many anchors.  Otherwise i is a primary itself."""
    pri = []
    for i, r in enumerate(regs):
        r.update(id=i, parent=UNSET, subsc=r.get("subsc", 0), n_sub=r.get("n_sub", 0), strand_retained=0)
    for i, r in enumerate(regs):
        if i == 0:
            r["parent"] = 0
            pri.append(0)
            continue
        si, ei = r["qs"], r["qe"]
        over = [j for j in pri if regs[j]["qe"] > si and regs[j]["qs"] < ei]
        uncov = (ei - si) - _union_len([(max(regs[j]["qs"], si), min(regs[j]["qe"], ei)) for j in over])
        for j in over:
            p = regs[j]
            ol = min(ei, p["qe"]) - max(si, p["qs"])
            lo, hi = min(ei - si, p["qe"] - p["qs"]), max(ei - si, p["qe"] - p["qs"])
            if F(F(ol) / F(lo)) - F(F(uncov) / F(hi)) > F(mask_level):
                r["parent"] = p["parent"]
                p["subsc"] = max(p["subsc"], r["score"])
                if r["cnt"] >= p["cnt"]:
                    p["n_sub"] += 1
                break
        else:
            r["parent"] = i
            r["n_sub"] = 0
            pri.append(i)
    return regs


def sync_regs(regs):
    """after regions left: id = the place in the list, parent follows its region there; a parent that left leaves UNSET"""
    where = {r["id"]: i for i, r in enumerate(regs) if r["id"] >= 0}
    for i, r in enumerate(regs):
        r["id"] = i
        r["parent"] = where.get(r["parent"], UNSET) if r["parent"] >= 0 else UNSET
    return regs


def select_sub(regs, pri_ratio, min_diff, best_n, min_strand_sc, in_place=True):
    """Keep the primaries (and inversions); keep a secondary while fewer than best_n are kept and its score is within pri_ratio or min_diff of
    its parent's - unless it has its parent's coordinates - or it lies on the other strand of the same stretch of reference with a score above
    min_strand_sc.  in_place: as upstream, the list is compacted while it is walked, so "the parent" is whatever stands at the parent's old
    place by then; False reads the parent as it was before the walk (the reading a reader of the definition would expect)."""
    if not (F(pri_ratio) > F(0)) or not regs:
        return regs
    before = [dict(r) for r in regs]
    r = regs
    k = n_2nd = 0
    n = len(r)
    for i in range(n):
        ri = r[i]
        p = (r if in_place else before)[ri["parent"]] if ri["parent"] != i else None
        keep = False
        if p is None or ri["inv"]:
            keep = True
        elif (F(ri["score"]) >= F(p["score"]) * F(pri_ratio) or ri["score"] + min_diff >= p["score"]) and n_2nd < best_n:
            if not all(ri[f] == p[f] for f in ("qs", "qe", "rid", "rs", "re")):
                keep = True
                n_2nd += 1
        elif n_2nd < best_n and ri["score"] > min_strand_sc and p["rev"] != ri["rev"] and p["rid"] == ri["rid"] and ri["rs"] < p["re"] and ri["re"] > p["rs"]:
            ri["strand_retained"] = 1
            keep = True
            n_2nd += 1
        if keep:
            r[k] = dict(ri)
            k += 1
    del r[k:]
    if k != n:
        sync_regs(r)
    return r


def chain_post(tab, mask_level, pri_ratio, min_diff, best_n, min_strand_sc, in_place=True):
    """set_parent + select_sub over a table of regions (dicts); each result carries `orig`, its row in the table"""
    regs = [dict(t, orig=i) for i, t in enumerate(tab)]
    set_parent(regs, mask_level)
    return select_sub(regs, pri_ratio, min_diff, best_n, min_strand_sc, in_place)
