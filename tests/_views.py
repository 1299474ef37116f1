"""Seeded L0 cases on sequence VIEWS (gamdp_task a_rc / b_rc / a_off / b_off), for tests/test_views_cpu.py and
tests/test_gpu_views.py.  CPU only.

The contract (include/gamdp.h): a view -- reverse complement first, then the suffix from `off` on -- gives exactly the result that an
explicitly reverse-complemented / chopped copy gives.  A case here is a plain L0 case on the COPIES (a, b, band, window, force flags:
what the oracle, which knows nothing of views, aligns) plus, per side, the view spec (rc, off) and the STORED sequence that goes into
the set, built so that view(stored) == copy byte for byte:

    stored = x                      (none)          stored = revcomp(x)              (rc)
    stored = prefix + x             (off)           stored = revcomp(prefix + x)     (rc + off)

All sequences are code bytes (A0 T1 C2 G3 N4).  The axes (see the module constants) are walked by counters, not drawn, so that every
value appears whatever the seed; the seed draws the bases.  Every case carries its axis values in case["tag"], which the tests put
into every assertion message.
"""
import hashlib
import os
import random
import re

SEED = 20261016
KINDS = ("none", "rc", "off", "rc+off")
KIND_PAIRS = [(ka, kb) for ka in KINDS for kb in KINDS]
OFF_RESIDUES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)
PREFIX_KINDS = ("random", "bait", "nbait")
NBAIT_DIST = (1, 63, 64, 65, 255, 256, 257, 320, 321)   # the N run ends this many bases before the view starts
BEGIN_MODES = ("0", "1", "band-1", "band", "band+1", "random")
N_MARGIN = 64                                            # gamdp_host.cpp prepare_task
_RC = bytes([1, 0, 3, 2, 4]) + bytes(range(5, 256))

# kernel cell -> (kernel name as gamdp_ctx_launch_info reports it, bands, N inside the window, environment of the process it needs)
CELLS = {
    "c17":    ("k_align<17,4,false>",    (512,),       False, {"GAMDP_NO_PAIR": "1"}),
    "c17n":   ("k_align<17,4,true>",     (512,),       True,  {}),
    "c5":     ("k_align<5,0,false>",     (150,),       False, {}),
    "c5n":    ("k_align<5,0,true>",      (150,),       True,  {}),
    "p17":    ("k_align_p<17,4>",        (512,),       False, {}),
    "o19":    ("k_align_o<19,15>",       (150,),       False, {"GAMDP_QUAD_MIN": "1"}),
    "q19":    ("k_align_q<19,15,false>", (150,),       False, {"GAMDP_QUAD_MIN": "1", "GAMDP_NO_PAIR": "1"}),
    "q19n":   ("k_align_q<19,15,true>",  (150,),       True,  {"GAMDP_QUAD_MIN": "1"}),
    "gen2":   ("k_align<2,-1,true>",     (1, 63),      None,  {}),
    "gen3":   ("k_align<3,-1,true>",     (64, 95),     None,  {}),
    "gen5":   ("k_align<5,-1,true>",     (96, 159),    None,  {}),
    "gen9":   ("k_align<9,-1,true>",     (160, 287),   None,  {}),
    "gen17":  ("k_align<17,-1,true>",    (288, 543),   None,  {}),
    "wide":   ("k_align_w",              (544, 2048),  None,  {}),
}
LONG_CELLS = ("c17", "p17", "c5", "o19", "q19", "c17n", "c5n")   # a >= 20 kb case each: strips, re-centring, ring refills behind a base != 0


def kernel_names_in_source():
    """The names in kernel_info (gam_ngs_amd/csrc/gamdp_kernel.hip), read from the table itself."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "gam_ngs_amd", "csrc", "gamdp_kernel.hip")).read()
    return set(re.findall(r'^\s*\{K_[A-Z0-9_]+,\s*"([^"]+)"', src, re.M))


def revcomp(codes):
    return bytes(codes).translate(_RC)[::-1]


def apply_view(stored, rc, off):
    """What the library's view (rc first, then the suffix) of `stored` is; None when off lies past the end (status INVALID)."""
    x = revcomp(stored) if rc else bytes(stored)
    return None if off > len(x) else x[off:]


def rand_codes(rng, n):
    return bytes(rng.getrandbits(2) for _ in range(n))


def mutate(rng, a, sub=0.03, ins=0.005, dele=0.005):
    out = bytearray()
    for ch in a:
        u = rng.random()
        if u < dele:
            continue
        out.append((ch + rng.randint(1, 3)) & 3 if (u < dele + sub and ch < 4) else ch)
        if rng.random() < ins:
            out.append(rng.getrandbits(2))
    return bytes(out) or b"\0"


def offsets_for(band):
    """The offsets of the residue axis: the residues themselves, one offset below the band, one above band + 64 * 17 (everything a
    kernel fetches in front of the view is then real sequence)."""
    return OFF_RESIDUES + (max(1, band - 3), band + 64 * 17 + 7)


def _prefix(rng, kind, off_a, off_b, dist, a, b):
    """(prefix_a, prefix_b) in view orientation.  bait: the last min(off_a, off_b) bases continue the homology backwards (an alignment
    that leaked to pos < 0 would score higher and start earlier); nbait: a run of N that ends `dist` bases before the view starts."""
    pa, pb = bytearray(rand_codes(rng, off_a)), bytearray(rand_codes(rng, off_b))
    if kind == "bait":
        m = min(off_a, off_b)
        if m:
            h = rand_codes(rng, m)
            pa[off_a - m:] = h
            pb[off_b - m:] = bytes((c + rng.randint(1, 3)) & 3 if rng.random() < 0.02 else c for c in h)
        else:   # one side only: the prefix is a copy of the head of the partner, the best a leak could find
            if off_a:
                k = min(off_a, len(b))
                pa[off_a - k:] = b[:k]
            if off_b:
                k = min(off_b, len(a))
                pb[off_b - k:] = a[:k]
    elif kind == "nbait":
        for p, off in ((pa, off_a), (pb, off_b)):
            if off >= dist:
                run = min(rng.randint(1, 40), off - dist + 1)
                for k in range(off - dist - run + 1, off - dist + 1):
                    p[k] = 4
    return bytes(pa), bytes(pb)


def rows_of(case):
    """x_size of the call (banded_smith_waterman.cc:91-95) for calls the DP runs; 0 otherwise."""
    la, lb, band = len(case["a"]), len(case["b"]), case["band"]
    if case["begin_b"] >= lb or case["end_b"] < case["begin_b"] or case["begin_a"] > la + band:
        return 0
    eb = min(case["end_b"], lb - 1)
    return max(0, min(eb - case["begin_b"] + 1, la + band - case["begin_a"], 500000))


def window_truth_n(case):
    """Does the window of the call, margin included, hold an N -- on the COPIES, base by base (the property the choice of kernel must
    respect: never the N-free kernel when this is true).  None when the pre-checks settle the call."""
    a, b, band = case["a"], case["b"], case["band"]
    X = case["rows"]
    if not X:
        return None
    lo, hi = case["begin_a"] - band - N_MARGIN, case["begin_a"] + X - 1 + band + N_MARGIN
    if 4 in a[max(lo, 0):max(hi + 1, 0)]:
        return True
    lo, hi = case["begin_b"] - N_MARGIN, case["begin_b"] + X - 1 + N_MARGIN
    return 4 in b[max(lo, 0):max(hi + 1, 0)]


def _one_case(rng, cell, band, ka, kb, want_n, n, prefix_kind, begin_mode, off_a, off_b, dist, tail):
    rate = 0.0 if band < 8 else (0.002 if band < 64 else 0.005)
    a = rand_codes(rng, n)
    b = mutate(rng, a, 0.03, rate, rate)
    begin_a = {"0": 0, "1": 1, "band-1": band - 1, "band": band, "band+1": band + 1}.get(begin_mode)
    if begin_a is None:
        begin_a = rng.randint(0, n // 3)
    begin_a = max(0, min(begin_a, n // 2))
    begin_b = max(0, begin_a + rng.randint(-min(band, 4), min(band, 4)))
    fs = fe = False
    if tail == "right":        # a right tail: force_start, to the last base of both views (PctgBuilder.cc:1573-1611)
        fs, end_a, end_b = True, n - 1, len(b) - 1
        begin_b = begin_a
    elif tail == "left":       # a left tail: force_end, the b window from base 0
        fe, begin_b = True, 0
        begin_a = min(begin_a, band)
        end_b = rng.randint(len(b) // 2, len(b) - 1)
        end_a = min(n - 1, begin_a + end_b)
    elif tail == "ends":       # to the last base of the views
        end_a, end_b = n - 1, len(b) - 1
    else:                      # a chain call: a frame of b against the window of a it maps to
        end_b = rng.randint(begin_b + (len(b) - begin_b) // 2, len(b) + 3)
        end_a = min(n + 2, begin_a + (end_b - begin_b) + rng.randint(-3, 3))
    case = dict(band=band, begin_a=begin_a, end_a=max(0, end_a), begin_b=begin_b, end_b=end_b, fs=fs, fe=fe)
    if want_n:   # runs of N inside what the DP touches, on both sequences
        a, b = bytearray(a), bytearray(b)
        for s, p0, p1 in ((a, begin_a, min(n, begin_a + (end_b - begin_b))), (b, begin_b, min(len(b), end_b))):
            for _ in range(rng.randint(1, 3)):
                p = rng.randint(p0, max(p0, p1 - 8))
                for k in range(p, min(len(s), p + rng.randint(1, 6))):
                    s[k] = 4
        a, b = bytes(a), bytes(b)
    oa = off_a if "off" in ka else 0
    ob = off_b if "off" in kb else 0
    pa, pb = _prefix(rng, prefix_kind, oa, ob, dist, a, b)
    sa = pa + a
    sb = pb + b
    va, vb = ("rc" in ka, oa), ("rc" in kb, ob)
    case.update(a=a, b=b, va=va, vb=vb, stored_a=revcomp(sa) if va[0] else sa, stored_b=revcomp(sb) if vb[0] else sb, cell=cell,
                kernel=CELLS[cell][0], group="main")
    case["rows"] = rows_of(case)
    case["tag"] = dict(seed=SEED, cell=cell, band=band, kinds=(ka, kb), off=(oa, ob), prefix=prefix_kind,
                       nbait_dist=dist if prefix_kind == "nbait" else None, begin=begin_mode, begin_a=begin_a, tail=tail, n=n, want_n=want_n)
    return case


def check_case(case, revcomp_fn=None):
    """view(stored) == copy, byte for byte, with the library's own reverse complement when given (api.reverse_complement)."""
    rcf = revcomp_fn or revcomp
    for side in "ab":
        rc, off = case["v" + side]
        st = case["stored_" + side]
        x = rcf(st) if rc else st
        assert x[off:] == case[side], (side, case["tag"])
        assert apply_view(st, rc, off) == case[side], (side, case["tag"])


def matrix_cases(seed=SEED):
    """The covering set: for every kernel cell, all 16 view-kind pairs at every band of the cell, the other axes walked by counters."""
    rng = random.Random(seed)
    out = []
    ctr = 0
    for cell, (name, bands, n_mode, env) in CELLS.items():
        reps = 2 if len(bands) == 1 else 1
        for band in bands:
            offs = offsets_for(band)
            for rep in range(reps):
                for ka, kb in KIND_PAIRS:
                    ctr += 1
                    want_n = bool(n_mode) if n_mode is not None else ctr % 3 == 0
                    # the N-free cells must stay N-free whatever the block granularity says: no N in their stored sequences at all
                    # (the N bait at those kernels is a group of its own: nbait_cases)
                    pk = PREFIX_KINDS[ctr % 3] if n_mode is not False else PREFIX_KINDS[ctr % 2]
                    off_a, off_b = offs[(ctr * 7 + 3) % len(offs)], offs[(ctr * 5 + 1) % len(offs)]
                    dist = NBAIT_DIST[(ctr // 3) % len(NBAIT_DIST)]
                    if pk == "nbait":   # the prefix has to hold the run
                        big = [o for o in offs if o >= dist]
                        if off_a < dist:
                            off_a = big[ctr % len(big)]
                        if off_b < dist:
                            off_b = big[(ctr // 2) % len(big)]
                    if off_a % 16 == off_b % 16:
                        off_b += 5      # the two sides never share a residue
                    n = rng.choice((300, 700, 1200)) if cell == "wide" else max(rng.choice((300, 800, 1500, 2500, 4000, 6000)), 2 * band + 40)
                    tail = ("right", "chain", "ends", "chain", "left", "chain", "right", "ends")[ctr % 8]
                    out.append(_one_case(rng, cell, band, ka, kb, want_n, n, pk, BEGIN_MODES[ctr % len(BEGIN_MODES)], off_a, off_b, dist, tail))
        if cell in LONG_CELLS:
            band = bands[0]
            offs = offsets_for(band)
            for k, (ka, kb) in enumerate((("rc+off", "off"), ("off", "rc+off"))):
                ctr += 1
                off_a, off_b = offs[(ctr * 3) % len(offs)], offs[-1] + 9 * k + 1
                if off_a % 16 == off_b % 16:
                    off_b += 5
                out.append(_one_case(rng, cell, band, ka, kb, bool(n_mode), 20000 + 1000 * k, "bait", BEGIN_MODES[(ctr + k) % 3],
                                     off_a, off_b, 1, ("right", "ends")[k]))
                out[-1]["tag"]["long"] = True
    return out


def nbait_cases(seed=SEED):
    """N bait at the N-free kernels: a run of N in the chopped-off prefix at every distance of NBAIT_DIST, none inside the view.  Whether
    the call runs the N-aware or the N-free kernel depends on the distance (the window's margin, the 256-base blocks of the N counts);
    the result may not.  A group of its own: in a batch with these the planner may merge the N-free calls into the N-aware launch."""
    rng = random.Random(seed + 1)
    out = []
    ctr = 0
    for cell in ("c5", "p17", "o19", "q19", "c17"):
        band = CELLS[cell][1][0]
        for dist in NBAIT_DIST:
            for ka, kb in (("off", "rc+off"), ("rc+off", "off"), ("off", "none"), ("rc", "rc+off")):
                ctr += 1
                offs = [o for o in offsets_for(band) if o >= dist]
                off_a, off_b = offs[ctr % len(offs)], offs[(ctr * 3 + 1) % len(offs)]
                if off_a % 16 == off_b % 16:
                    off_b += 3
                c = _one_case(rng, cell, band, ka, kb, False, rng.choice((400, 900, 2000)), "nbait", BEGIN_MODES[ctr % len(BEGIN_MODES)],
                              off_a, off_b, dist, ("right", "ends", "chain")[ctr % 3])
                c["group"] = "nbait"
                out.append(c)
    return out


def degenerate_cases():
    """Views of nothing or almost nothing: off == len, off == len - 1, off > len (status INVALID, prepare_task), rc of a length-1 and
    a length-0 sequence.  The expected status is the oracle's on the copies, or INVALID where no copy exists."""
    rng = random.Random(SEED + 2)
    x, y = rand_codes(rng, 200), rand_codes(rng, 180)
    one, none = b"\2", b""
    out = []
    for band in (5, 150, 512, 600):
        for fs, fe in ((False, False), (True, False), (False, True)):
            for name, sa, va, sb, vb in (
                    ("a off==len", x, (False, 200), y, (False, 0)), ("b off==len", x, (False, 0), y, (True, 180)),
                    ("a off==len-1", x, (True, 199), y, (False, 3)), ("b off==len-1", x, (False, 16), y, (False, 179)),
                    ("a off>len", x, (False, 201), y, (False, 0)), ("b off>len rc", x, (True, 0), y, (True, 181)),
                    ("a off>>len", x, (True, 1 << 40), y, (False, 0)),
                    ("rc of length 1", one, (True, 0), y, (True, 0)), ("rc of length 1, b", x, (False, 0), one, (True, 0)),
                    ("rc of length 0", none, (True, 0), y, (False, 0)), ("rc of length 0, b", x, (True, 5), none, (True, 0)),
                    ("length 1 off 1", one, (True, 1), one, (False, 1))):
                for ba, bb in ((0, 0), (1, 0), (0, 1)):
                    out.append(dict(stored_a=sa, va=va, stored_b=sb, vb=vb, band=band, begin_a=ba, end_a=250, begin_b=bb, end_b=250, fs=fs, fe=fe,
                                    tag=dict(name=name, band=band, fs=fs, fe=fe, begin=(ba, bb))))
    return out


def digest(cases):
    """A digest of a case list: a changed generator changes it."""
    h = hashlib.sha256()
    for c in cases:
        h.update(repr((c["stored_a"], c["va"], c["stored_b"], c["vb"], c["band"], c["begin_a"], c["end_a"], c["begin_b"], c["end_b"],
                       c["fs"], c["fe"])).encode())
    return h.hexdigest()[:16]


# ---- the Python mirror of npre_window_has_n (gamdp_dev.h), for the N-by-window assertions on launches ----------------

def npre(stored):
    """N counts per 256 bases of a stored sequence, forward orientation; None when it holds no N (SeqSet::npre)."""
    if 4 not in stored:
        return None
    pre = [0] * ((len(stored) + 255) // 256 + 1)
    for k, c in enumerate(stored):
        pre[k // 256 + 1] += c == 4
    for k in range(1, len(pre)):
        pre[k] += pre[k - 1]
    return pre


def block_answer(stored, rc, off, lo, hi):
    """What the library answers for bases [lo, hi] of the view: by blocks of 256 bases of the stored sequence."""
    pre = npre(stored)
    if pre is None:
        return False
    n = len(stored)
    o_lo, o_hi = off + max(lo, 0), min(off + hi, n - 1)
    if o_lo > o_hi:
        return False
    f_lo, f_hi = (n - 1 - o_hi, n - 1 - o_lo) if rc else (o_lo, o_hi)
    return pre[f_hi // 256 + 1] != pre[f_lo // 256]


def call_block_answer(case, view=True):
    """The library's choice for the view call (or the copy call) of a case: True = N-aware."""
    X, band = case["rows"], case["band"]
    sa, (arc, aoff) = (case["stored_a"], case["va"]) if view else (case["a"], (False, 0))
    sb, (brc, boff) = (case["stored_b"], case["vb"]) if view else (case["b"], (False, 0))
    return block_answer(sa, arc, aoff, case["begin_a"] - band - N_MARGIN, case["begin_a"] + X - 1 + band + N_MARGIN) or \
        block_answer(sb, brc, boff, case["begin_b"] - N_MARGIN, case["begin_b"] + X - 1 + N_MARGIN)
