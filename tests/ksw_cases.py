"""Cases for the two device alignment kernels (csrc/sh_align.h ksw_extd2_core, csrc/sh_long.h lr_ksw_ll_wave), shared by the CPU and
GPU suites: the smallest shapes on both sides of every border at which the kernels change path, with sequences built to make the
maximum tie, z-drop fire and the band clip.  Seeded and deterministic.

The module also restates, from the rules in the kernels' comments alone, which storage form a case must take on each route, the widest
rounded range over its anti-diagonals and how many steps of the cell loop that makes.  tests/test_ksw_cases_cpu.py checks that the table
reaches every combination that can exist; tests/test_ksw_gpu.py runs it on the device against the oracle."""
import numpy as np

# a, b, sc_ambi, q, e, q2, e2 of the presets sr, map-ont, map-hifi (tests/golden/make_align_golden.py)
SCORES = [(2, 8, 1, 12, 2, 24, 1), (2, 4, 1, 4, 2, 24, 1), (1, 4, 1, 6, 2, 26, 1)]

EZ_RIGHT, EZ_APPROX_MAX, EZ_APPROX_DROP, EZ_EXTZ_ONLY, EZ_REV_CIGAR = 0x02, 0x08, 0x10, 0x40, 0x80
FLAGS = [0, 0x40, 0x40 | 0x02 | 0x80, 0x02, 0x08, 0x08 | 0x10, 0x40 | 0x08 | 0x10]

# the kernel's constants (sh_align.h)
AL_T16, AL_Q16, AL_P, AL_WIDE_MIN = 448, 336, 4096, 128

EZ_FIELDS = ("max", "zdropped", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q", "score", "reach_end", "n_cigar")


# ---- what the kernels' comments say about a case, in plain Python ------------------------------------------------------------
def n_col(qlen, tlen, w):
    ww = max(qlen, tlen) if w < 0 else w
    return ((min(qlen, tlen, ww + 1) + 15) // 16 + 1) * 16


def p_need(qlen, tlen, w):
    """direction bytes: one row of n_col per anti-diagonal"""
    return (qlen + tlen - 1) * n_col(qlen, tlen, w)


def form(route, qlen, tlen, w):
    """0: DP state and direction bytes in LDS; 1: state in LDS, directions in HBM; 2: both in HBM.  The state stays in LDS up to
    AL_T16 target and AL_Q16 query bases (rounded to 16), the directions up to AL_P bytes; the long-read stage (route 1) never
    keeps the directions in LDS."""
    t16, q16 = (tlen + 15) // 16 * 16, (qlen + 15) // 16 * 16
    mem_lds = t16 <= AL_T16 and q16 <= AL_Q16
    if route == 0 and mem_lds and p_need(qlen, tlen, w) <= AL_P:
        return 0
    return 1 if mem_lds else 2


def ranges(qlen, tlen, w):
    """(st0, en0, st, en) of every anti-diagonal the kernel computes: the band's [st0, en0] and what it is rounded to (st down to a
    multiple of 16, en up to one less than a multiple of 16); the walk ends where the band leaves the matrix."""
    ww = max(qlen, tlen) if w < 0 else w
    out = []
    for r in range(qlen + tlen - 1):
        st, en = max(0, r - qlen + 1, (r - ww + 1) >> 1), min(tlen - 1, r, (r + ww) >> 1)
        if st > en:
            break
        out.append((st, en, st // 16 * 16, (en + 16) // 16 * 16 - 1))
    return out


def widest(qlen, tlen, w):
    return max(en - st + 1 for _, _, st, en in ranges(qlen, tlen, w))


def loop_class(qlen, tlen, w):
    """("narrow" | "wide", steps): the wider cell loop (four cells a lane, 256 a step) takes the diagonals whose rounded range exceeds
    AL_WIDE_MIN cells; the narrow one moves 64 a step.  The class of a case is that of its widest diagonal."""
    n = widest(qlen, tlen, w)
    return ("wide", (n + 255) // 256) if n > AL_WIDE_MIN else ("narrow", (n + 63) // 64)


# ---- sequences ---------------------------------------------------------------------------------------------------------------
def _fit(seq, n, rng):
    seq = list(seq)[:n]
    return np.array(seq + [int(x) for x in rng.integers(0, 4, n - len(seq))], np.uint8)


def _mutate(src, rng, sub=0.06, indel=0.04):
    out = []
    for c in src:
        r = rng.random()
        if r < sub:
            out.append(int(rng.integers(0, 4)))
        elif r < sub + indel / 2:
            continue
        elif r < sub + indel:
            out += [int(c), int(rng.integers(0, 4))]
        else:
            out.append(int(c))
    return out


def _repeat(unit, n, phase=0):
    u = len(unit)
    return np.array([unit[(i + phase) % u] for i in range(n)], np.uint8)


def make_pair(kind, qlen, tlen, rng):
    """query, target (codes 0..4) of the given lengths"""
    if kind == "unrelated":
        return rng.integers(0, 4, qlen).astype(np.uint8), rng.integers(0, 4, tlen).astype(np.uint8)
    if kind in ("related", "ambi", "noisy"):
        t = rng.integers(0, 4, tlen).astype(np.uint8)
        q = _fit(_mutate(t, rng, 0.12, 0.10) if kind == "noisy" else _mutate(t, rng), qlen, rng)
        if kind == "ambi":
            for s in (q, t):
                s[rng.integers(0, len(s), max(1, len(s) // 25))] = 4
        return q, t
    if kind == "prefix":      # the first third matches, the rest is unrelated: an extension has to stop there
        t = rng.integers(0, 4, tlen).astype(np.uint8)
        k = max(1, min(qlen, tlen) // 3)
        return _fit(t[:k], qlen, rng), t
    if kind == "recover":     # a match, then stretches in which a substitution is paid back exactly: the maximum is reached again and again
        t = rng.integers(0, 4, tlen).astype(np.uint8)
        q = _fit(t, qlen, rng)
        for p in range(min(qlen, tlen) // 2, min(qlen, tlen) - 1, 5):
            q[p] = (q[p] + 1) & 3
        return q, t
    if kind == "twopath":
        # A shared start, then 24 bases of ACAC.. in the query against CACA.. in the target, then tails that match nothing.  The diagonal
        # scores mismatches; one base off it on EITHER side everything matches, so from a few bases in, every other anti-diagonal holds its
        # new maximum in two neighbouring cells, and the last of them is the final maximum.  The scan's lane class of a cell is its distance
        # from the query's end modulo 4 (the diagonal starts where the query ends), so tails of 16, 17, 18, 19 bases - chosen by the
        # length modulo 4 - put that pair on every pair of neighbouring classes: (0,1), (1,2), (2,3), (3,0).
        assert qlen == tlen and qlen >= 64
        g = 16 + (qlen & 3)
        head = rng.integers(0, 4, qlen - 24 - g).astype(np.uint8)
        q = np.concatenate([head, _repeat([0, 1], 24), np.full(g, 3, np.uint8)])
        t = np.concatenate([head, _repeat([1, 0], 24), np.full(g, 2, np.uint8)])
        return q, t
    unit = {"homo": [0], "ac": [0, 1], "rep5": [0, 2, 2, 1, 3]}.get(kind)
    if kind == "rep171":
        unit = [int(x) for x in np.random.default_rng(171).integers(0, 4, 171)]
    assert unit is not None, kind
    q, t = _repeat(unit, qlen), _repeat(unit, tlen, int(rng.integers(0, len(unit))) if len(unit) > 1 and rng.random() < 0.5 else 0)
    if rng.random() < 0.5 and qlen > 8:      # a few substitutions, so that the repeat's copies differ in score
        q[rng.integers(0, qlen, max(1, qlen // 40))] = (unit[0] + 1) & 3
    return q, t


KINDS = ["related", "unrelated", "prefix", "homo", "ac", "rep5", "rep171", "ambi", "recover", "noisy"]

# ---- the extension alignment: shapes (qlen, tlen, w) on both sides of every border --------------------------------------------
SQUARES = [1, 15, 16, 17, 63, 64, 65,      # one narrow step
           80, 127, 128,                    # two narrow steps: the left neighbour crosses lane 63
           129, 144, 200, 256,              # one wide step
           257, 272, 320, 336]              # two wide steps: the left neighbour crosses the dword of lane 63
BANDS_400 = [127, 128, 129, 255, 256, 257, 3]
UNEQUAL = [(1, 300), (300, 1), (40, 400), (400, 40)]
P_BORDER = [(32, 32, -1), (33, 33, -1), (64, 65, 5), (65, 65, 5)]      # direction bytes on both sides of AL_P
STATE_BORDER = [(300, 448), (300, 449), (336, 400), (337, 400)]         # state in LDS / in HBM: AL_T16, AL_Q16
HBM_NARROW = [(400, 400, 80), (500, 460, 100), (350, 500, 40), (460, 300, 20)]      # both in HBM with one and with several narrow steps
BIG = (700, 900, -1)                                                    # route 1 only


def shapes():
    s = [(n, n, -1) for n in SQUARES] + [(400, 400, w) for w in BANDS_400] + [(q, t, -1) for q, t in UNEQUAL] + P_BORDER
    return s + [(q, t, -1) for q, t in STATE_BORDER] + HBM_NARROW


# one shape of every (form, loop) pair, for the families that are not crossed with every shape
REPRESENTATIVES = [(30, 34, -1), (40, 44, -1), (100, 100, -1), (128, 128, -1), (200, 200, -1), (320, 320, -1), (400, 400, 40), (400, 400, 100), (400, 400, 200), (400, 460, -1)]


def _case(name, kind, qlen, tlen, w, sc, flag, zdrop, end_bonus, routes, seed):
    rng = np.random.default_rng(seed)
    q, t = make_pair(kind, qlen, tlen, rng)
    a, b, amb, go, ge, go2, ge2 = SCORES[sc]
    return {"name": name, "kind": kind, "query": q, "target": t, "a": a, "b": b, "sc_ambi": amb, "q": go, "e": ge, "q2": go2, "e2": ge2,
            "w": w, "zdrop": zdrop, "end_bonus": end_bonus, "flag": flag, "routes": routes, "family": name.split(":")[0]}


def extd2_cases():
    cases, n = [], 0
    for i, (ql, tl, w) in enumerate(shapes()):      # every shape: global and extension, sequence kinds and score sets taking turns
        for j, flag in enumerate((0, 0x40)):
            for kind in (KINDS[(i + 3 * j) % len(KINDS)], "related" if (i + j) % 2 else "noisy"):
                n += 1
                cases.append(_case(f"shape:{ql}x{tl}w{w}:{kind}:f{flag:#x}", kind, ql, tl, w, (i + j) % 3, flag, -1, 10 if flag & 0x40 else -1, (0, 1), 1000 + n))
    for i, (ql, tl, w) in enumerate(REPRESENTATIVES):      # every flag on every storage form and both loops
        for j, flag in enumerate(FLAGS):
            for k, kind in enumerate(("related", "noisy", "recover")):
                n += 1
                cases.append(_case(f"flags:{ql}x{tl}w{w}:{kind}:f{flag:#x}", kind, ql, tl, w, (i + j + k) % 3, flag, (-1, 400, 100)[(j + k) % 3], (-1, 10)[(i + j + k) % 2], (0, 1), 3000 + n))
    for i, (ql, tl, w) in enumerate([(60, 64, -1), (150, 150, -1), (200, 260, 151), (300, 300, -1), (400, 400, 151), (400, 460, -1)]):      # z-drop
        for j, kind in enumerate(("prefix", "unrelated", "related", "noisy", "rep5")):
            for k, zdrop in enumerate((100, 400)):
                n += 1
                flag = (0x40, 0, 0x08 | 0x10, 0x40 | 0x08 | 0x10, 0x40 | 0x02 | 0x80)[(i + j + k) % 5]
                cases.append(_case(f"zdrop:{ql}x{tl}w{w}:{kind}:z{zdrop}:f{flag:#x}", kind, ql, tl, w, (i + j) % 3, flag, zdrop, (10, -1)[k], (0, 1), 5000 + n))
    for i, (ql, tl, w) in enumerate([(63, 65, -1), (128, 130, -1), (129, 129, -1), (257, 257, -1), (400, 400, 128), (337, 449, -1)]):      # ties of the maximum
        for j, kind in enumerate(("homo", "ac", "rep5", "rep171", "recover")):
            n += 1
            cases.append(_case(f"ties:{ql}x{tl}w{w}:{kind}", kind, ql, tl, w, (i + j) % 3, (0x40, 0)[j % 2], (-1, 100)[(i + j) % 2], 10, (0, 1), 7000 + n))
    for i, base in enumerate((64, 152, 300, 420)):      # ties between two lane classes of the scan, every pair of neighbours
        for d in range(4):
            n += 1
            flag, zdrop = ((0x40, 100), (0x40, -1), (0, -1))[(i + d) % 3]
            cases.append(_case(f"ties:{base + d}x{base + d}w-1:twopath", "twopath", base + d, base + d, -1, (i + d) % 3, flag, zdrop, 10 if flag else -1, (0, 1), 8000 + n))
    ql, tl, w = BIG
    cases.append(_case(f"big:{ql}x{tl}w{w}:related:f0x40", "related", ql, tl, w, 1, 0x40, 400, 10, (1,), 9001))
    cases.append(_case(f"big:{ql}x{tl}w{w}:noisy:f0x0", "noisy", ql, tl, w, 2, 0, -1, -1, (1,), 9002))
    return cases


_EXTD2 = None


def extd2_table():
    """the table, built once and never changed by its users"""
    global _EXTD2
    if _EXTD2 is None:
        _EXTD2 = extd2_cases()
    return _EXTD2


# ---- the local alignment ------------------------------------------------------------------------------------------------------
LL_QLEN = [1, 7, 8, 9, 56, 63, 64, 65, 72, 504, 512, 513]      # qlen % 8 (the padding) and the padded length % 64 (the chunk carry of F)
LL_TLEN = [1, 2, 64, 300]
LL_SCORES = [(2, 4, 1, 4, 2), (1, 4, 1, 6, 2), (2, 8, 1, 12, 2)]      # a, b, sc_ambi, gapo, gape


def ll_cases():
    cases, n = [], 0
    kinds = ["inside", "related", "unrelated", "homo", "ac", "rep5", "rep171", "ambi"]
    for i, ql in enumerate(LL_QLEN):
        for j, tl in enumerate(LL_TLEN):
            for k in range(2):
                n += 1
                kind = kinds[(i + 2 * j + 5 * k) % len(kinds)]
                rng = np.random.default_rng(11000 + n)
                if kind == "inside":      # the query is a stretch of the target that ends inside it: the maximum sits in the last column
                    t = rng.integers(0, 4, tl).astype(np.uint8)
                    s = int(rng.integers(0, max(1, tl - ql)))
                    q = _fit(t[s:s + ql], ql, rng)
                else:
                    q, t = make_pair(kind, ql, tl, rng)
                a, b, amb, go, ge = LL_SCORES[(i + j + k) % 3]
                cases.append({"name": f"ll:{ql}x{tl}:{kind}", "query": q, "target": t, "a": a, "b": b, "sc_ambi": amb, "gapo": go, "gape": ge})
    return cases


_LL = None


def ll_table():
    global _LL
    if _LL is None:
        _LL = ll_cases()
    return _LL


# ---- the oracle on a case (ctypes; the structure of oracle/mm_align.h) -----------------------------------------------------------
def oracle_extd2(L, c):
    """mma_ksw_extd2 with the case's arguments: ({field: value}, [cigar words])"""
    import ctypes as C

    class Ez(C.Structure):
        _fields_ = [("max", C.c_uint32), ("zdropped", C.c_int), ("max_q", C.c_int), ("max_t", C.c_int), ("mqe", C.c_int), ("mqe_t", C.c_int),
                    ("mte", C.c_int), ("mte_q", C.c_int), ("score", C.c_int), ("reach_end", C.c_int), ("n_cigar", C.c_int), ("m_cigar", C.c_int),
                    ("cigar", C.POINTER(C.c_uint32))]
    mat = np.zeros(25, np.int8)
    L.mma_gen_simple_mat(5, mat.ctypes.data, c["a"], c["b"], c["sc_ambi"])
    ez = Ez()
    q, t = np.ascontiguousarray(c["query"], np.uint8), np.ascontiguousarray(c["target"], np.uint8)
    L.mma_ksw_extd2(len(q), q.ctypes.data, len(t), t.ctypes.data, 5, mat.ctypes.data, c["q"], c["e"], c["q2"], c["e2"], c["w"], c["zdrop"], c["end_bonus"], c["flag"], C.byref(ez))
    vals = {f: int(getattr(ez, f)) for f in EZ_FIELDS}
    vals["max"] = int(np.int32(np.uint32(ez.max)))
    cig = [int(ez.cigar[i]) for i in range(ez.n_cigar)]
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.cast(ez.cigar, C.c_void_p))      # the oracle leaves the CIGAR to its caller
    return vals, cig


def oracle_ll(L, c):
    import ctypes as C
    L.mma_ksw_ll.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.mma_ksw_ll.restype = C.c_int
    mat = np.zeros(25, np.int8)
    L.mma_gen_simple_mat(5, mat.ctypes.data, c["a"], c["b"], c["sc_ambi"])
    q, t = np.ascontiguousarray(c["query"], np.uint8), np.ascontiguousarray(c["target"], np.uint8)
    qe, te = C.c_int(), C.c_int()
    sc = L.mma_ksw_ll(len(q), q.ctypes.data, len(t), t.ctypes.data, mat.ctypes.data, c["gapo"], c["gape"], C.byref(qe), C.byref(te))
    return int(sc), qe.value, te.value
