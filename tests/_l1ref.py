"""The reference's own merge-block driver (oracle/_ref/libgaml1ref.so: PctgBuilder::alignMergeBlock and the four
functions it calls, cut out of the reference's PctgBuilder.cc at build time, behind oracle/ref_l1_shim.cc), and the
answer format that tests/golden/l1_vs_ref.json.gz stores for one merge block.

An answer is a dict:
  thrown      the reference threw (std::out_of_range from Contig::at: status 2)
  align_ok, coords_set, align_rev, m_start, m_end, s_start, s_end
              what alignMergeBlock left in the MergeBlock (coordinates only when it wrote them)
  n_dp        find_alignment calls made
  cells       sum of the fill sizes of those calls (the L0 oracle's x_size * y_size of each recorded window: the
              reference does not report it; the L0 oracle is pinned to the reference's find_alignment)
  trail_crc   CRC32 of the trail, the list of every call's result in call order in OracleResult.key() layout
  trail       (a subset of the answers only) the full trail: per call [a_tag, a_off, b_tag, b_off, begin_a, end_a,
              begin_b, end_b, force_start, force_end] + key; a_tag / b_tag name the contig ('M' master, 'S' slave,
              'R' the slave's reverse complement), a_off / b_off the start of a tail cut from it
"""
import ctypes as C
import json
import os
import zlib

import _oracle as O

PATH = os.path.join(O.ORACLE_DIR, "_ref", "libgaml1ref.so")
TRAIL_CAP = 64


class RefCall(C.Structure):
    _fields_ = [("a_tag", C.c_char), ("b_tag", C.c_char), ("force_start", C.c_uint8), ("force_end", C.c_uint8),
                ("status", C.c_uint8), ("first_found", C.c_uint8), ("last_found", C.c_uint8), ("pad_", C.c_uint8),
                ("a_off", C.c_uint64), ("b_off", C.c_uint64),
                ("begin_a", C.c_uint64), ("end_a", C.c_uint64), ("begin_b", C.c_uint64), ("end_b", C.c_uint64),
                ("r_begin_a", C.c_uint64), ("r_begin_b", C.c_uint64), ("r_a_size", C.c_uint64), ("r_b_size", C.c_uint64),
                ("length", C.c_uint64), ("n_match", C.c_uint64), ("score", C.c_int64), ("homology", C.c_double),
                ("first_a", C.c_uint64), ("first_b", C.c_uint64), ("last_a", C.c_uint64), ("last_b", C.c_uint64)]

    def key(self):
        """the call's result in OracleResult.key() layout (as tests/_oracle.py ref_key maps the L0 reference's)"""
        if self.status != 0:
            return (O.OUT_OF_RANGE if self.status == 2 else O.INVALID, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0)
        st = O.EMPTY if (self.length == 0 and self.r_a_size == 0 and self.r_b_size == 0) else O.OK
        return (st, self.r_begin_a, self.r_begin_b, self.score, self.n_match, self.length, self.first_a, self.first_b,
                self.first_found, self.last_a, self.last_b, self.last_found, self.homology)

    def window(self):
        return [self.a_tag.decode(), self.a_off, self.b_tag.decode(), self.b_off, self.begin_a, self.end_a,
                self.begin_b, self.end_b, self.force_start, self.force_end]


_lib = None


def lib():
    """the L1 reference library, or None where it was not built (no reference tree, e.g. on the GPU box)"""
    global _lib
    if _lib is None:
        if not os.path.exists(PATH):
            return None
        l = C.CDLL(PATH)
        l.gamref_align_merge_block.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(O.OracleBlock),
                                               C.c_uint32, C.POINTER(O.OracleMB), C.POINTER(RefCall), C.c_uint32]
        l.gamref_align_merge_block.restype = C.c_int
        l.gamref_l1_sources_sha256.restype = C.c_char_p
        _lib = l
    return _lib


def blocks_array(sc):
    nb = len(sc["blocks"])
    arr = (O.OracleBlock * max(1, nb))()
    for k, b in enumerate(sc["blocks"]):
        arr[k].m_begin, arr[k].m_end, arr[k].s_begin, arr[k].s_end = b[0], b[1], b[2], b[3]
        arr[k].m_strand, arr[k].s_strand, arr[k].n_reads = b[4].encode(), b[5].encode(), b[6]
    return arr


def trail_crc(keys):
    return zlib.crc32(json.dumps([[float(x) if isinstance(x, float) else int(x) for x in k] for k in keys]).encode())


def views(sc):
    """code arrays of the contigs a trail's tags name"""
    m, s = O.encode(sc["master"]), O.encode(sc["slave"])
    buf = C.create_string_buffer(s, max(1, len(s)))
    O.oracle().gamdp_oracle_revcomp(buf, len(s))
    return {"M": m, "S": s, "R": buf.raw[:len(s)]}


def ref_mb(sc, lib_=None):
    """(OracleMB-layout outcome, [RefCall]) of the reference's alignMergeBlock on one scenario"""
    l = lib_ or lib()
    mb = O.OracleMB()
    mb.m_ltail, mb.m_rtail, mb.s_ltail, mb.s_rtail = [int(x) for x in sc["tails"]]
    trail = (RefCall * TRAIL_CAP)()
    m, s = sc["master"].encode(), sc["slave"].encode()
    l.gamref_align_merge_block(m, len(m), s, len(s), blocks_array(sc), len(sc["blocks"]), C.byref(mb), trail, TRAIL_CAP)
    assert mb.n_dp <= TRAIL_CAP, mb.n_dp
    return mb, [trail[i] for i in range(mb.n_dp)]


def answer(sc, full_trail=False, lib_=None):
    """the stored form of the reference's answer (see the module docstring)"""
    mb, trail = ref_mb(sc, lib_)
    v = views(sc)
    cells = 0
    for t in trail:  # the fill size of each recorded window, as the L0 oracle counts it
        if t.a_tag in b"MSR" and t.b_tag in b"MSR":
            a, b = v[t.a_tag.decode()][t.a_off:], v[t.b_tag.decode()][t.b_off:]
            r, _ = O.oracle_align(a, b, 150, t.begin_a, t.end_a, t.begin_b, t.end_b, t.force_start, t.force_end,
                                  want_ops=False)
            assert r.key() == t.key(), ("the L0 oracle differs from the reference on a recorded call", r.key(), t.key())
            cells += r.cells
    keys = [t.key() for t in trail]
    out = dict(thrown=mb.status == 2, status=mb.status, align_ok=bool(mb.align_ok), coords_set=bool(mb.touched),
               align_rev=bool(mb.align_rev) if mb.touched else False,
               m_start=mb.m_start, m_end=mb.m_end, s_start=mb.s_start, s_end=mb.s_end,
               n_dp=mb.n_dp, cells=cells, trail_crc=trail_crc(keys))
    if full_trail:
        out["trail"] = [t.window() + list(t.key()) for t in trail]
    return out
