"""findHits queries for gamdp_find_hits_batch: the tail windows of a tests/_gage.py problem, and a Python statement of
ABlast::findHits that also returns the vote count of the hits (ablast.cc:41-76; max_score is not observable through the
host's list)."""
import numpy as np

M64 = (1 << 64) - 1


def _ends(mb, slen):
    """(rev, sa, ea, sb, eb): the chain's orientation by read majority and its ends on the master and on the slave view,
    taken from the outer blocks of the merge block (the driver takes them from the chain's alignments)."""
    con = sum(b[6] for b in mb["blocks"] if b[4] == b[5])
    dis = sum(b[6] for b in mb["blocks"] if b[4] != b[5])
    rev = con < dis
    sa, ea = min(b[0] for b in mb["blocks"]), max(b[1] for b in mb["blocks"])
    s0, s1 = min(b[2] for b in mb["blocks"]), max(b[3] for b in mb["blocks"])
    sb, eb = (slen - 1 - s1, slen - 1 - s0) if rev else (s0, s1)
    return rev, sa, ea, sb, eb


def tail_queries(pb, word=20):
    """-> (seqs, queries).  seqs: the master contigs, then the slave contigs, as code bytes.  queries: the left and right
    tail findHits calls of every merge block, shaped as gamdp_l1.cpp builds them (PctgBuilder.cc:1535-1611): tuples
    (a_id, a_rc, a_off, a_start, a_end, b_id, b_rc, b_off, b_start, b_end, word)."""
    master, slave = pb["master"], pb["slave"]
    seqs = [c["seq"].tobytes() for c in master] + [c["seq"].tobytes() for c in slave]
    nm = len(master)
    queries = []
    for g in pb["graphs"]:
        for lst in g:
            for mb in lst:
                m, s = mb["m_id"], nm + mb["s_id"]
                mlen, slen = master[mb["m_id"]]["n"], slave[mb["s_id"]]["n"]
                rev, sa, ea, sb, eb = _ends(mb, slen)
                if sa > 0 and sb > 0:   # left tails: force_end, both windows from base 0
                    if sa < sb:
                        queries.append((s, rev, 0, 0, sb - 1, m, False, 0, 0, sa - 1, word))
                    else:
                        queries.append((m, False, 0, 0, sa - 1, s, rev, 0, 0, sb - 1, word))
                ti, tj = mlen - 1 - ea, slen - 1 - eb
                if ti > 0 and tj > 0:   # right tails: a chop_begin view of one contig against the rest of the other
                    if ti < tj:
                        queries.append((s, rev, eb + 1, 0, slen - eb - 2, m, False, 0, ea + 1, mlen - 1, word))
                    else:
                        queries.append((m, False, ea + 1, 0, mlen - ea - 2, s, rev, 0, eb + 1, slen - 1, word))
    return seqs, queries


def view(codes, rc, off):
    """the code bytes of a gamdp view: reverse complement first, then the suffix from off"""
    c = np.frombuffer(codes, dtype=np.uint8)
    if rc:
        c = np.array([1, 0, 3, 2, 4], dtype=np.uint8)[np.minimum(c, 4)][::-1]
    return c[off:].tobytes()


def py_find_hits(a, a_s, a_e, b, b_s, b_e, word):
    """(hits, votes) of ABlast(word).findHits on code bytes"""
    alen, blen = len(a), len(b)
    a_s, a_e, b_s, b_e = a_s & M64, a_e & M64, b_s & M64, b_e & M64
    if alen == 0 or blen == 0:
        return [], 0
    a_e, b_e = min(a_e, alen - 1), min(b_e, blen - 1)
    if a_s > a_e or b_s > b_e or a_e + 1 < word + a_s or b_e + 1 < word + b_s or word == 0:
        return [], 0

    def codes(s, first, last):
        out = []
        for p in range(first, last + 1):
            c = 0
            for i in range(p, p + word):
                c = (4 * c + s[i]) & M64
            out.append(c)
        return out

    pos = {}
    for ia, c in enumerate(codes(a, a_s, a_e - word + 1)):
        pos.setdefault(c, []).append(ia)
    f = [0] * (a_e - a_s + 1)
    for ib, c in enumerate(codes(b, b_s, b_e - word + 1)):
        for ia in pos.get(c, ()):
            if ia >= ib:
                f[ia - ib] += 1
    best = max(f)
    if best == 0:
        return [], 0
    return [(a_s + i) & 0xFFFFFFFF for i, v in enumerate(f) if v == best], best
