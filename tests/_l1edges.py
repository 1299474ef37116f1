"""Hand-built merge blocks at the edges of the L1 driver's rules (PctgBuilder::alignMergeBlock / findBestAlignment /
alignBlocks / is_good, reference PctgBuilder.cc:726-844, 1361-1731), in the scenario format of tests/_l1cases.py.

Every case is built for one rule; the stored reference answers (tests/golden/l1_vs_ref.json.gz) say what the reference
did with it, and tests/test_l1_oracle_vs_ref.py checks that the cases still reach what they were built for.  The
generator is separate from tests/_l1cases.py so that the random stream of the existing scenarios stays as it is.

  hom95 / hom94          main chain of one call at exactly 95 % homology (n_match * 100 == 95 * length) and one match
                         short, then the same in chains of three calls (is_good(vector))
  thr / thr-1            min(i1, j1) and min(i2, j2) equal to the tail threshold and one less, at threshold 200 (long
                         contigs), 100 (alignMergeBlock's own threshold) and 0.3 * size (contigs under 334 bases)
  tail-len               tails homologous over 0.7 * min(i, j) bases (left_min_len / right_min_len) and a few bases
                         either side, poly-A against poly-C beyond: the tail call (forced at both ends) spans the whole
                         tail, so these reach the homology edge of is_good(single) around 70 %, not its length edge
  tail-empty             a demanded tail that cannot align (all N against bases): MyAlignment() or MyAlignment(100)
  tie / no-reads         concordant and discordant reads equal (con_prob == 0.5), and no reads at all (0 / 0)
  vote-wrong             every block votes for the wrong orientation: the retry finds the alignment
  rev-tails              reversed slaves with only one slave tail flag set (s_ltail / s_rtail swap)
  left-rev / right-rev   the slave's tail longer than the master's (is_left_rev / is_right_rev)
  order                  first and last block out of master order; a middle block beyond both
  edge0 / edge-end       frames starting at base 0 and ending at size - 1
  past-end               a frame running past the end of the master (the reference throws)
  single                 one-base frames
  short-frame            a frame shorter than 100 bases (min_frame_len)
  adjacent / overlap / clamp
                         consecutive blocks with no gap, overlapping, and an empty first call followed by an
                         overlapping block (last_match + gap < 0 is clamped to 0)

Line coverage of the five reference functions over these cases together with the seeded and GAGE-shaped groups
(tests/golden/make_golden_l1_vs_ref.py --coverage): every line of alignMergeBlock, findBestAlignment, alignBlocks and
both is_good overloads that gcov counts is reached (228 of 228 lines).  The second `return true;` of is_good(vector)
(PctgBuilder.cc:1723) follows a return; gcov does not count it as a line.
"""
import random

import _cases
from _l1cases import revcomp_str

BASES = "ACGT"


def _rand(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def _subst(rng, s, positions):
    s = list(s)
    for p in positions:
        s[p] = rng.choice([b for b in BASES if b != s[p]])
    return "".join(s)


def _spread(n_sub, length):
    """n_sub positions evenly inside [length / (2 n_sub), length): far enough from the ends that the local alignment
    keeps every mismatch"""
    step = length / float(n_sub + 1)
    return [int(step * (k + 1)) for k in range(n_sub)]


def _sc(kind, master, slave, blocks, tails=(True, True, True, True)):
    return dict(kind=kind, master=master, slave=slave, blocks=[tuple(b) for b in blocks], tails=tuple(bool(t) for t in tails))


def _homology_cases(rng):
    out = []
    for length, n_sub in ((100, 5), (100, 6), (200, 10), (200, 11), (60, 3), (60, 4), (140, 7), (140, 8)):
        kind = "hom95" if n_sub * 100 == 5 * length else "hom94"
        core = _rand(rng, length)
        core_s = _subst(rng, core, _spread(n_sub, length))
        for tails in ((False,) * 4, (True,) * 4):
            ml, sl, mr, sr = _rand(rng, 300), _rand(rng, 300), _rand(rng, 300), _rand(rng, 300)
            out.append(_sc("%s-one-%d" % (kind, length), ml + core + mr, sl + core_s + sr,
                           [(300, 300 + length - 1, 300, 300 + length - 1, "+", "+", 10)], tails))
    # chains of three calls: every call at 95 %, or one call one match short
    for bad in (None, 0, 1, 2):
        parts_m, parts_s, blocks, pos = [], [], [], 250
        lead_m, lead_s = _rand(rng, 250), _rand(rng, 250)
        for k in range(3):
            core = _rand(rng, 100)
            parts_m.append(core)
            parts_s.append(_subst(rng, core, _spread(6 if k == bad else 5, 100)))
            blocks.append((pos, pos + 99, pos, pos + 99, "+", "+", 10))
            gap = _rand(rng, 40)
            parts_m.append(gap)
            parts_s.append(gap)
            pos += 140
        out.append(_sc("hom%s-chain" % ("95" if bad is None else "94-%d" % bad), lead_m + "".join(parts_m) + _rand(rng, 250),
                       lead_s + "".join(parts_s) + _rand(rng, 250), blocks, (False,) * 4))
    return out


def _tailed(rng, kind, li, lj, ri, rj, core_len=600, hom_left=None, hom_right=None, tails=(True,) * 4, div=0.0, fill=False):
    """master = left tail (li) + core + right tail (ri), slave likewise (lj, rj); the tails are homologous over
    hom_left / hom_right bases next to the core (all of the shorter tail if None), unrelated beyond (poly-A on the
    master against poly-C on the slave with fill, so that the tail alignment stops exactly where the homology ends)"""
    core = _rand(rng, core_len)
    core_s = _cases.mutate(rng, core, 0.01 * div, 0.0, 0.0) if div else core

    def tail_pair(n_m, n_s, hom):
        hom = min(n_m, n_s) if hom is None else min(hom, n_m, n_s)
        shared = _rand(rng, hom)
        if fill:
            return "A" * (n_m - hom) + shared, "C" * (n_s - hom) + shared
        return _rand(rng, n_m - hom) + shared, _rand(rng, n_s - hom) + shared
    mL, sL = tail_pair(li, lj, hom_left)
    mR, sR = tail_pair(ri, rj, hom_right)
    mR, sR = mR[::-1], sR[::-1]
    master, slave = mL + core + mR, sL + core_s + sR
    return _sc(kind, master, slave, [(li, li + core_len - 1, lj, lj + core_len - 1, "+", "+", 20)], tails)


def _threshold_cases(rng):
    out = []
    # long contigs: findBestAlignment's threshold is 200, alignMergeBlock's 100
    for t in (200, 199, 100, 99, 150):
        out.append(_tailed(rng, "thr-left-%d" % t, t, t + 30, 5, 5))
        out.append(_tailed(rng, "thr-right-%d" % t, 5, 5, t + 30, t))
        out.append(_tailed(rng, "thr-both-%d" % t, t, t, t, t))
    # contigs under 334 bases: 0.3 * size < 100, both thresholds are int(0.3 * size)
    for size in (300, 250, 200, 120):
        for d in (0, -1):
            core_len = size - 2 * (int(0.3 * size) + d) if size >= 200 else size // 3
            t = (size - core_len) // 2
            out.append(_tailed(rng, "thr-small-%d%+d" % (size, d), t, t, size - core_len - t, size - core_len - t,
                               core_len=core_len))
    return out


def _tail_len_cases(rng):
    out = []
    for n in (300, 400):
        want = int(0.7 * n)
        for hom in range(want - 3, want + 3):
            out.append(_tailed(rng, "tail-len-left-%d-%d" % (n, hom), n, n + 20, 3, 3, hom_left=hom, fill=True))
            out.append(_tailed(rng, "tail-len-right-%d-%d" % (n, hom), 3, 3, n + 20, n, hom_right=hom, fill=True))
    return out


def _special_cases(rng):
    out = []
    # a demanded tail that cannot align: N against bases
    for side in ("left", "right"):
        sc = _tailed(rng, "tail-empty-" + side, 300, 320, 300, 320, hom_left=0, hom_right=0)
        m = sc["master"]
        sc["master"] = "N" * 300 + m[300:] if side == "left" else m[:len(m) - 300] + "N" * 300
        out.append(sc)
    # orientation votes
    for rev in (False, True):
        base = _tailed(rng, "x", 50, 50, 50, 50, core_len=800)
        m, s = base["master"], base["slave"]
        blocks = [(50, 449, 50, 449), (450, 849, 450, 849)]
        if rev:
            s = revcomp_str(s)
            n = len(s)
            blocks = [(mb, me, n - 1 - se, n - 1 - sb) for mb, me, sb, se in blocks]
        st = "-" if rev else "+"
        out.append(_sc("tie-%s" % ("rev" if rev else "fwd"), m, s,
                       [blocks[0] + ("+", st, 10), blocks[1] + ("+", "-" if st == "+" else "+", 10)]))
        out.append(_sc("no-reads-%s" % ("rev" if rev else "fwd"), m, s, [b + ("+", st, 0) for b in blocks]))
        out.append(_sc("vote-wrong-%s" % ("rev" if rev else "fwd"), m, s,
                       [b + ("+", "+" if rev else "-", 7) for b in blocks]))
    # reversed slaves with one slave tail flag; the slave's tail longer than the master's (left_rev / right_rev)
    for li, lj, ri, rj in ((250, 320, 250, 320), (320, 250, 320, 250), (250, 320, 320, 250)):
        for tails in ((True, True, True, False), (True, True, False, True), (True, True, True, True)):
            sc = _tailed(rng, "rev-tails-%d-%d-%d-%d-%s" % (li, lj, ri, rj, "".join("1" if t else "0" for t in tails)),
                         li, lj, ri, rj, tails=tails)
            s = revcomp_str(sc["slave"])
            n = len(s)
            sc["slave"] = s
            sc["blocks"] = [(b[0], b[1], n - 1 - b[3], n - 1 - b[2], "+", "-", b[6]) for b in sc["blocks"]]
            out.append(sc)
            out.append(_tailed(rng, "lr-rev-%d-%d-%d-%d-%s" % (li, lj, ri, rj, "".join("1" if t else "0" for t in tails)),
                               li, lj, ri, rj, tails=tails))
    # block order: reversed list, and a middle block beyond the first and the last
    base = _tailed(rng, "x", 100, 100, 100, 100, core_len=1200, div=1.0)
    m, s = base["master"], base["slave"]
    bl = [(100, 399, 100, 399, "+", "+", 9), (500, 799, 500, 799, "+", "+", 9), (900, 1199, 900, 1199, "+", "+", 9)]
    out.append(_sc("order-reversed", m, s, bl[::-1]))
    out.append(_sc("order-middle-last", m, s, [bl[0], bl[2], bl[1]]))
    # frames on the contig ends, past the end, one base long, shorter than 100
    core = _rand(rng, 700)
    core_s = _cases.mutate(rng, core, 0.01, 0.0, 0.0)
    n = len(core_s)
    out.append(_sc("edge0-edge-end", core, core_s, [(0, 699, 0, n - 1, "+", "+", 10)]))
    out.append(_sc("edge0-two", core, core_s, [(0, 299, 0, 299, "+", "+", 10), (400, 699, 400, n - 1, "+", "+", 10)]))
    out.append(_sc("past-end-master", core, core_s, [(0, 299, 0, 299, "+", "+", 10), (400, 760, 400, n - 1, "+", "+", 10)]))
    out.append(_sc("past-end-slave", core, core_s, [(100, 699, 100, n + 40, "+", "+", 10)]))
    for b0, e0 in ((650, 1300), (699, 900), (600, 2000)):
        out.append(_sc("past-end-%d-%d" % (b0, e0), core, core_s, [(100, 399, 100, 399, "+", "+", 10), (b0, e0, b0, n - 1, "+", "+", 10)]))
    out.append(_sc("single-base", core, core_s, [(350, 350, 350, 350, "+", "+", 10)]))
    out.append(_sc("single-base-last", core, core_s, [(100, 299, 100, 299, "+", "+", 10), (699, 699, n - 1, n - 1, "+", "+", 3)]))
    for flen in (40, 99, 100):
        out.append(_sc("short-frame-%d" % flen, core, core_s, [(200, 199 + flen, 200, 199 + flen, "+", "+", 10)]))
        out.append(_sc("short-frame-%d-chain" % flen, core, core_s,
                       [(100, 399, 100, 399, "+", "+", 10), (450, 449 + flen, 450, 449 + flen, "+", "+", 10)]))
    # consecutive blocks: no gap, overlapping, and an empty first call (last_match (0, 0)) before an overlapping block
    out.append(_sc("adjacent", core, core_s, [(100, 299, 100, 299, "+", "+", 10), (300, 599, 300, 599, "+", "+", 10)]))
    out.append(_sc("overlap", core, core_s, [(100, 349, 100, 349, "+", "+", 10), (300, 599, 300, 599, "+", "+", 10)]))
    junk = _rand(rng, 60)
    out.append(_sc("clamp", junk + core, _rand(rng, 60) + core_s,
                   [(0, 59, 0, 59, "+", "+", 10), (0, 400, 0, 400, "+", "+", 10)]))
    out.append(_sc("empty-slave-frame", core, core_s, [(0, 199, 0, -1, "+", "+", 10), (250, 599, 250, 599, "+", "+", 10)]))
    return out


def cases(seed=2024):
    rng = random.Random(seed)
    return _homology_cases(rng) + _threshold_cases(rng) + _tail_len_cases(rng) + _special_cases(rng)
