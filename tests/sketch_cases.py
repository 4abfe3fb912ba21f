"""The case table of the minimizer sketch and seeding front ends, shared by tests/test_sketch_cases_cpu.py (which proves from the oracle alone
that the table reaches what it is meant to) and tests/test_sketch_gpu.py (which runs it on the device).  Everything is seeded.  Lengths are the
smallest that still reach the code: one block of W steps is 5..19 bases, a read of the read kernel at most 1024, a sketch segment of a long
read 256 and of the reference 1024.

Beside the table: a plain numpy statement of "every k-mer of a sequence" (kmers), the tie-aware brute force built on it (window_minima), a
Python restatement of the sketch state machine that also says at which step and by which rule each push is made (py_sketch: only used to
show that a case reaches a rule), and the numpy statement of mm_seed_mz_flt (thin)."""
import numpy as np

WS = (5, 10, 11, 19)                 # the instantiated windows
KS = (5, 7, 15, 19, 21, 23)          # every form
K_WIDE = 27                          # SketchState and SketchStateDyn only
SEED_CAP = 192                       # seed records per read of the read kernel (sh_ctx::seed_cap)
LSEG, REF_SEG = 256, 1024            # bases per sketch segment: long reads, reference
LT_CAP = 2048                        # k_long_probe: distinct hashes of the over-full bins of one read
REC_PREV_SAME = 1 << 30
# what the front-end tests run: (preset, w, k) for the read kernel, (w, k) for the long front end (all four instantiated windows),
# and the thinning options of the satellite reads
K1_CFG = (("sr", 11, 21), ("map-ont", 10, 15), ("map-ont", 19, 19))
LONG_WK = ((10, 15), (5, 7), (11, 21), (19, 19))
THIN_MID_OCC, THIN_Q_OCC_FRAC = 8, 0.01
ACGT = np.frombuffer(b"ACGT", np.uint8)

# Hand-checkable, and a rule the set view of minimizers does not give.  w = 5, k = 5; the k-mers by end position (hash, strand):
#    4 (891,0)  5 (581,1)  6 (34,1)  7 (34,0)  8 (2,0)  9 (315,1)  10 (209,0)  11 (702,0)  12 (47,0)  13 (499,0)  14 (110,1)  15 (414,0)
#    16 (943,0)  17 (700,0)
# GGATC (ends at 6) and GATCC (ends at 7) are reverse complements: one hash, 34, on opposite strands.  Step 7 takes (34, 7) as the new minimum
# (<=, rightmost on ties) while l = 8 < w + k - 1, so (34, 6) is not pushed there.  Step 8 is the first full window (l = 9 = w + k - 1): its
# special case pushes every other entry of the window with the hash of the minimum AS IT STANDS BEFORE THIS STEP'S K-MER IS LOOKED AT, i.e. of
# the stale minimum (34, 7): that is (34, 6).  Then (2, 8) becomes the minimum; since l < w + k the old minimum (34, 7) is dropped unpushed.
# The first full window is positions 4..8 and its minimum is (2, 8): (34, 6) is the minimum of no full window, yet it is emitted.
# (2, 8) leaves the window at step 13 and is pushed, the rescan finds (47, 12); that leaves at step 17 and is pushed, the rescan finds
# (110, 14), which the end of the sequence flushes.
KAT_SEQ, KAT_W, KAT_K = b"GCGGATCCCGGCAAGCAT", 5, 5
KAT_MINIMIZERS = [(34, 6, 1), (2, 8, 0), (47, 12, 0), (110, 14, 1)]


def _rng(*key):
    return np.random.default_rng([0x5CE7C4] + [int(v) for v in key])


def rand_seq(rng, n):
    return bytes(ACGT[rng.integers(0, 4, n)])


def mutate(rng, s, subs):
    s = bytearray(s)
    for _ in range(subs):
        p = int(rng.integers(0, len(s)))
        s[p] = b"ACGT"[(b"ACGT".index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return bytes(s)


def tandem(rng, period, n, subs=0):
    unit = rand_seq(rng, period)
    return mutate(rng, (unit * (n // period + 1))[:n], subs)


def revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


# ---- plain statements ---------------------------------------------------------------------------------------------------------------------
def nt4(seq):
    """codes 0..3 for A C G T/U in either case, 4 for every other byte: written out, not taken from any table of the code under test"""
    a = np.frombuffer(bytes(seq), np.uint8)
    code = np.full(len(a), 4, np.uint8)
    for letters, c in ((b"Aa", 0), (b"Cc", 1), (b"Gg", 2), (b"TtUu", 3)):
        for ch in letters:
            code[a == ch] = c
    return code


def hash64(key, mask):
    """minimap2's invertible mix on 2k bits, over a uint64 array"""
    key = key.astype(np.uint64)
    m = np.uint64(mask)
    s = lambda v: np.uint64(v)
    key = (~key + (key << s(21))) & m
    key = key ^ key >> s(24)
    key = ((key + (key << s(3))) + (key << s(8))) & m
    key = key ^ key >> s(14)
    key = ((key + (key << s(2))) + (key << s(4))) & m
    key = key ^ key >> s(28)
    key = (key + (key << s(31))) & m
    return key


def kmers(seq, k):
    """(hash, strand, valid) by END position, for every position of seq; valid: the k bases ending there are all unambiguous (k odd)"""
    code = nt4(seq)
    n = len(code)
    h, z, ok = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, bool)
    if n < k:
        return h, z, ok
    c = code.astype(np.uint64) & np.uint64(3)
    f, r = np.zeros(n - k + 1, np.uint64), np.zeros(n - k + 1, np.uint64)
    for j in range(k):      # base j of the k-mer that starts at i
        f |= c[j:j + n - k + 1] << np.uint64(2 * (k - 1 - j))
        r |= (np.uint64(3) - c[j:j + n - k + 1]) << np.uint64(2 * j)
    amb = np.concatenate(([0], np.cumsum(code == 4)))
    good = (amb[k:] - amb[:n - k + 1]) == 0
    assert not np.any(good & (f == r)), "odd k: no k-mer is its own reverse complement"
    mask = (1 << 2 * k) - 1
    h[k - 1:] = hash64(np.minimum(f, r), mask)
    z[k - 1:] = (f > r).astype(np.uint8)
    ok[k - 1:] = good
    return h, z, ok


def has_window_tie(seq, w, k):
    """the same hash twice among w consecutive positions (what the tie rules are about)"""
    h, _, ok = kmers(seq, k)
    for d in range(1, w):
        if np.any(ok[d:] & ok[:-d] & (h[d:] == h[:-d])) if len(h) > d else False:
            return True
    return False


def window_minima(seq, w, k):
    """N-free sequences: the rightmost minimum of every full window of w k-mers, as a set of (hash, end position, strand).  Ties allowed."""
    h, z, ok = kmers(seq, k)
    assert ok[k - 1:].all()
    hv = h[k - 1:]
    if len(hv) < w:
        return set()
    win = np.lib.stride_tricks.sliding_window_view(hv, w)
    at = np.arange(len(win)) + (w - 1 - np.argmin(win[:, ::-1], axis=1))      # rightmost
    return {(int(hv[i]), int(i) + k - 1, int(z[i + k - 1])) for i in np.unique(at)}


def py_sketch(seq, w, k):
    """The sketch state machine, restated in Python with the same statement order: [(hash, pos, strand, step, rule)] where step is the base at
    which the push is made and rule is 'first' (first-window tie loop), 'new' (new minimum pushes the old), 'left' (the minimum left the
    window), 'tie' (tie loop after a rescan) or 'end'.  Used to show which rules a case reaches; checked against the oracle on the whole table."""
    code = nt4(seq)
    mask, shift1 = (1 << 2 * k) - 1, 2 * (k - 1)
    MAXV = (1 << 64) - 1
    bx, by = [MAXV] * w, [MAXV] * w
    minx = miny = MAXV
    kf = kr = l = bp = mp = 0
    out = []
    hcache = {}

    def hx(v):
        if v not in hcache:
            hcache[v] = int(hash64(np.array([v], np.uint64), mask)[0])
        return hcache[v]

    def push(x, y, i, rule):
        out.append((x >> 8, y >> 1, y & 1, i, rule))

    for i, c in enumerate(code.tolist()):
        ix = iy = MAXV
        if c < 4:
            kf = (kf << 2 | c) & mask
            kr = kr >> 2 | (3 ^ c) << shift1
            z = 0 if kf < kr else 1
            l += 1
            if l >= k:
                ix, iy = hx(kr if z else kf) << 8 | k, i << 1 | z
        else:
            l = 0
        bx[bp], by[bp] = ix, iy
        if l == w + k - 1 and minx != MAXV:
            for j in list(range(bp + 1, w)) + list(range(bp)):
                if bx[j] == minx and by[j] != miny:
                    push(bx[j], by[j], i, "first")
        if ix <= minx:
            if l >= w + k and minx != MAXV:
                push(minx, miny, i, "new")
            minx, miny, mp = ix, iy, bp
        elif bp == mp:
            if l >= w + k - 1 and minx != MAXV:
                push(minx, miny, i, "left")
            minx = MAXV
            for j in list(range(bp + 1, w)) + list(range(bp + 1)):
                if minx >= bx[j]:
                    minx, miny, mp = bx[j], by[j], j
            if l >= w + k - 1 and minx != MAXV:
                for j in list(range(bp + 1, w)) + list(range(bp + 1)):
                    if bx[j] == minx and by[j] != miny:
                        push(bx[j], by[j], i, "tie")
        bp = bp + 1 if bp + 1 < w else 0
    if minx != MAXV:
        push(minx, miny, len(code), "end")
    return out


def oracle_sketch(O, seq, w, k):
    """the oracle's minimizers of seq in emission order: (hash uint64[], y uint32[] = pos << 1 | strand)"""
    if len(seq) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    x, y = O.sketch(bytes(seq), w, k)
    assert np.all((x & np.uint64(0xff)) == np.uint64(k))
    return x >> np.uint64(8), (y & np.uint64(0xffffffff)).astype(np.uint32)


def thin(hashes, mid_occ, q_occ_frac):
    """mm_seed_mz_flt as a statement: which minimizers of a read stay (bool per minimizer).  The product of n and the fraction is taken in
    single precision, as minimap2 and the kernel take it."""
    n = len(hashes)
    if n <= mid_occ or q_occ_frac <= 0:
        return np.ones(n, bool)
    _, inv, cnt = np.unique(hashes, return_inverse=True, return_counts=True)
    c = cnt[inv]
    lim = np.float32(n) * np.float32(q_occ_frac)
    return ~((c > mid_occ) & (c.astype(np.float32) > lim))


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def byte_reads(w, k):
    """every byte value 0..255 as a base, each behind w + k valid bases, in reads of at most 1024"""
    rng = _rng(7, w, k)
    unit, out, cur = w + k + 1, [], bytearray()
    for v in range(256):
        if len(cur) + unit + w + k > 1024:
            out.append(bytes(cur) + rand_seq(rng, w + k))
            cur = bytearray()
        cur += rand_seq(rng, w + k) + bytes([v])
    out.append(bytes(cur) + rand_seq(rng, w + k))
    return out


def sequences(w, k):
    """[(name, bytes)]: every case of at most 1024 bases - all three forms and the read kernel take them"""
    if (w, k) in _CACHE:
        return _CACHE[(w, k)]
    rng = _rng(1, w, k)
    T = []
    for n in (0, 1, k - 1, k, k + 1, k + w - 2, k + w - 1, k + w, 2 * (w + k), 150, 255, 256, 257, 1023, 1024):
        T.append((f"len_{n}", rand_seq(rng, n)))
    T.append(("kat", KAT_SEQ))
    # ties: homopolymers, tandem repeats, random sequence at small k (the table is built per k), palindromes
    for b in b"ACGT":
        T.append((f"homo_{chr(b)}", bytes([b]) * (3 * (w + k) + 1)))
    for period in sorted(set(range(1, 13)) | {w - 1, w, w + 1}):
        for subs in (0, 1, 2):
            T.append((f"tandem_p{period}_s{subs}", tandem(rng, period, 3 * (w + k) + 7, subs)))
    for i in range(24):
        T.append((f"random_{i}", rand_seq(rng, 120 + 7 * i)))
    for i in range(4):
        u = rand_seq(rng, k)
        T.append((f"palindrome_{i}", rand_seq(rng, w + k + i) + u + revcomp(u) + rand_seq(rng, w + k)))
    # ambiguous bases
    L = 2 * (w + k) + 3
    for name, base in (("rep", tandem(rng, 7, L, 2)), ("rnd", rand_seq(rng, L))):
        for p in range(L):
            T.append((f"n_slide_{name}_{p}", base[:p] + b"N" + base[p + 1:]))
    for run in sorted({1, k - 1, k, w, w + k}):
        for name, base in (("rep", tandem(rng, 5, 4 * (w + k), 1)), ("rnd", rand_seq(rng, 4 * (w + k)))):
            at = w + k + 3
            T.append((f"n_run{run}_{name}", base[:at] + b"N" * run + base[at:]))
    base = tandem(rng, 9, 60, 2) + rand_seq(rng, 60)
    T.append(("n_lead", b"NNN" + base))
    T.append(("n_trail", base + b"NN"))
    T.append(("n_both", b"N" + base + b"N"))
    T.append(("lower", base.lower()))
    T.append(("mixed_case", bytes(c | 0x20 if i % 3 == 0 else c for i, c in enumerate(base))))
    T.append(("uracil", base.replace(b"T", b"U")))
    T.append(("uracil_lower", base.lower().replace(b"t", b"u")))
    iu = bytearray(base)
    for i, ch in enumerate(b"RYKMSWBDHVNrykmswbdhvn-*.X"):
        iu[(5 * i + 2) % len(iu)] = ch
    T.append(("iupac", bytes(iu)))
    for i, s in enumerate(byte_reads(w, k)):
        T.append((f"bytes_{i}", s))
    # queue pressure: a homopolymer pushes at every step, W a block against 4 drained
    for n in (150, 1024):
        for unit in (b"A", b"C", b"AC", b"GT", b"AT"):
            T.append((f"queue_{unit.decode()}_{n}", (unit * n)[:n]))
    # around the read kernel's room for seed records: a homopolymer of n bases has about n - k minimizers
    for n in range(k + SEED_CAP - 4, k + SEED_CAP + 4):
        T.append((f"cap_{n}", b"G" * n))
    names = [n for n, _ in T]
    assert len(set(names)) == len(names) and all(len(s) <= 1024 for _, s in T)
    _CACHE[(w, k)] = T
    return T


def seam_reads(w, k, seg=LSEG):
    """Reads (or contigs) around the segment seams of a segment-parallel sketch (seg = 256: k_long_sketch, 1024: k_ref_sketch).  A segment
    starts from a clean state `warm` = w + k bases early and drops the pushes made before its first base `start`."""
    key = ("seam", w, k, seg)
    if key in _CACHE:
        return _CACHE[key]
    rng = _rng(2, w, k, seg)
    warm, D = w + k, w + k + 2
    T = []
    for j in (1, 2, 3):      # lengths around each seam: the last segment is empty, one base, ..., and `finish` runs in the right one
        for d in range(-D, D + 1):
            T.append((f"seam_len_{j}_{d}", rand_seq(rng, seg * j + d)))
    n = 3 * seg + seg // 2
    for d in range(-D, D + 1):      # a tie cluster (short tandem repeat) centred at every offset around all three seams
        s = bytearray(rand_seq(rng, n))
        for j in (1, 2, 3):
            period = 1 + (d + j) % 4
            c = seg * j + d
            lo = c - (w + k) // 2 - 2
            s[lo:lo + w + k + 4] = tandem(rng, period, w + k + 4)
        T.append((f"seam_tie_{d}", bytes(s)))
    # an N at start - warm puts the first full window of the run behind it (and its tie loop) at step start - 1, one at start - warm + 1 at start
    for name, off in (("start-1", -1), ("start-warm-1", -warm - 1), ("start-warm", -warm), ("start-warm+1", -warm + 1), ("start", 0)):
        for flavour in ("rnd", "rep2", "rep3"):
            s = bytearray(rand_seq(rng, n) if flavour == "rnd" else tandem(rng, int(flavour[3]), n, n // 200))
            for j in (1, 2, 3):
                s[seg * j + off] = ord("N")
            T.append((f"seam_n_{name}_{flavour}", bytes(s)))
    # ties across every seam; a pure repeat pushes with its own period, so its phases move every push of the cycle onto the seam
    for unit in (b"A", b"AC", b"ACG", b"AACG", b"AACCG", b"ACGGTCA"):
        for phase in range(len(unit)):
            T.append((f"seam_rep_{unit.decode()}_{phase}", (unit * (n + 8))[phase:phase + n]))
    _CACHE[key] = T
    return T


def satellite_reads(w, k, mid_occ=8):
    """Reads for the long front end's thinning screen (mm_seed_mz_flt at a small mid_occ): satellites whose unit gives each hash more than
    mid_occ copies and more than q_occ_frac of the read, clean reads, a read with a satellite inside, the heavily loaded table (more than
    LT_CAP / 2 distinct hashes in over-full bins: thinned in place), and one with more than LT_CAP of them, which no table of LT_CAP slots
    holds: that read has to leave for the re-sketch path."""
    key = ("sat", w, k, mid_occ)
    if key in _CACHE:
        return _CACHE[key]
    rng = _rng(3, w, k)
    T = [("empty", b"")]
    for i, (unit, n) in enumerate(((37, 3000), (64, 2500), (101, 4000), (13, 1500), (200, 5000))):
        T.append((f"sat_{unit}", tandem(rng, unit, n, 3 + i)))
    for i in range(3):
        T.append((f"clean_{i}", rand_seq(rng, 1500 + 700 * i)))
    T.append(("sat_inside", rand_seq(rng, 1500) + tandem(rng, 29, 1200, 2) + rand_seq(rng, 1300)))
    T.append(("short", rand_seq(rng, 40)))
    T.append(("tiny", rand_seq(rng, k - 1)))               # no minimizer, no seed: decided by the front end
    copies = mid_occ + 1
    u = rand_seq(rng, 6200)
    T.append(("table_loaded", u * copies))                 # about 55 kb
    u = rand_seq(rng, 12500)
    T.append(("table_over", u * copies))
    _CACHE[key] = T
    return T
