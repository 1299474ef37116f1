"""tests/_opsrunmodel.py -- the arithmetic of the walk that writes an edit string a diagonal run at a time (gamdp_ctx_set_ops_walk,
GAMDP_OPS_WALK_RUNS) -- against the reference's recorded edit strings and against hand-built paths.  No GPU: the GPU tests
(test_gpu_ops_walk.py) compare the device with the oracle and take the ops_by_run / ops_by_step split from here."""
import random
import zlib

import pytest

import _golden
import _opsrunmodel as M
import _oracle as O

CAPS = ("1", "15", "16", "17", "length-1", "length", "length+16")


def caps_of(length):
    named = {"length-1": length - 1, "length": length, "length+16": length + 16}
    return [max(0, int(c) if c.isdigit() else named[c]) for c in CAPS]


def check(ops, begin_a, begin_b, a, b, band, tba, tbb, caps, **kw):
    """the model's bytes are the string reversed and clipped, nothing behind the cap is touched, the split is the definition's"""
    seen = None
    for cap in caps:
        m = M.replay(ops, begin_a, begin_b, a, b, band, tba, tbb, cap=cap, **kw)
        assert m["bytes"] == M.expected_bytes(ops, cap), (cap, len(ops))
        assert m["length"] == len(ops) == m["ops_by_run"] + m["ops_by_step"]
        assert (m["ops_by_run"], m["ops_by_step"]) == M.split(ops, begin_a, begin_b, tbb)
        assert sum(m["run_lengths"]) == m["ops_by_run"] and len(m["run_lengths"]) == m["runs"]
        key = (m["ops_by_run"], m["ops_by_step"], m["runs"], m["run_lengths"])
        assert seen in (None, key), "the cap changes no step"
        seen = key
    return m


def golden_cases():
    out = []
    for name, cs, e in _golden.l0_cases():
        out.append((name, cs, e, e.get("ops")))
    assert len(out) == 673
    for d, cs, e in _golden.adversarial_cases():
        out.append((d["kind"], cs, e, e.get("ops")))
    return out


def test_golden_and_adversarial_strings_at_every_cap():
    n_ok = n_runs = 0
    for k, (name, cs, e, ops) in enumerate(golden_cases()):
        if e["status"] != O.OK:
            continue
        a, b = O.encode(cs["a"]), O.encode(cs["b"])
        if ops is None:   # recorded as a checksum: the oracle's string, checked against it
            _, ops = O.oracle_align(a, b, cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])
            assert zlib.crc32(ops.encode()) == e["ops_crc32"], name
        assert len(ops) == e["length"]
        caps = caps_of(len(ops)) if len(ops) <= 4000 else caps_of(len(ops))[2:5]
        m = check(ops, e["begin_a"], e["begin_b"], a, b, cs["band"], cs["begin_a"], cs["begin_b"], caps, C=(2, 3, 5, 9, 17, 19)[k % 6],
                  a_base=(7 * k) % 16, b_base=(11 * k + 3) % 16)
        n_ok += 1
        n_runs += m["runs"]
    assert n_ok >= 500 and n_runs >= 500   # (the other cases have no alignment and no string)


def test_where_a_run_is_cut_changes_no_byte():
    rng = random.Random(5)
    for name, cs, e, ops in golden_cases()[::7]:
        if e["status"] != O.OK or ops is None or len(ops) < 40:
            continue
        a, b = O.encode(cs["a"]), O.encode(cs["b"])
        want = M.expected_bytes(ops, len(ops))
        for depth in (1, 2, 16):
            for C in (2, 17):
                m = M.replay(ops, e["begin_a"], e["begin_b"], a, b, cs["band"], cs["begin_a"], cs["begin_b"], C=C, depth=depth,
                             a_base=rng.randrange(64), b_base=rng.randrange(64))
                assert m["bytes"] == want
                assert (m["ops_by_run"], m["ops_by_step"]) == M.split(ops, e["begin_a"], e["begin_b"], cs["begin_b"])


def diagonal_case(rng, n, lead=40, n_at_a=(), n_at_b=(), mism=()):
    """a path of `lead` diagonal steps, one GAP_B, and n diagonal steps up to the end cell: the run of n is the first the walk meets"""
    core = bytes(rng.getrandbits(2) for _ in range(lead + n))
    a = bytearray(core[:lead] + bytes([0]) + core[lead:])
    b = bytearray(core)
    ops = ["M"] * lead + ["B"] + ["M"] * n
    for i in mism:          # step i of the run, from its top
        k = len(b) - 1 - i
        b[k] = (b[k] + 1) & 3
        ops[len(ops) - 1 - i] = "X"
    for i in n_at_a:
        a[len(a) - 1 - i] = 4
    for i in n_at_b:
        b[len(b) - 1 - i] = 4
    return "".join(ops), bytes(a), bytes(b)


@pytest.mark.parametrize("n", (1, 15, 16, 17, 255, 256, 257))
def test_runs_of_the_edge_lengths(n):
    rng = random.Random(n)
    ops, a, b = diagonal_case(rng, n, mism=[i for i in (0, 14, 15, 16, n - 1) if i < n])
    for C, r_shift in ((17, 0), (5, 3), (2, 11)):
        m = check(ops, 0, 0, a, b, 20, 0, 0, caps_of(len(ops)), C=C, a_base=r_shift, b_base=5)
        assert sum(m["run_lengths"]) == len(ops) - 2   # (the gap and the step from x == 0, pos == 0 are single steps)
        assert m["run_lengths"][0] == n if n <= 17 else max(m["run_lengths"]) <= 256 and len(m["run_lengths"]) >= 3


def test_every_chunk_alignment():
    """(hi_a - 15) & 15 and (hi_b - 15) & 15 through all 16 x 16 values: the bases of the two packed planes move against each other"""
    rng = random.Random(16)
    ops, a, b = diagonal_case(rng, 70, mism=(0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 69))
    seen = set()
    for a_base in range(16):
        for b_base in range(16):
            m = check(ops, 0, 0, a, b, 20, 0, 0, (len(ops), 17), a_base=a_base, b_base=b_base)
            seen.add(((a_base + len(a) - 1 - 15) & 15, (b_base + len(b) - 1 - 15) & 15))
            assert m["run_lengths"][0] == 70
    assert len(seen) == 256


def test_a_run_that_ends_where_x_or_pos_reaches_one():
    rng = random.Random(3)
    core = bytes(rng.getrandbits(2) for _ in range(90))
    # the path is the main diagonal of a window that begins at (0, 0): the run stops on x == 0 == pos, the last step is a single one
    m = check("M" * 90, 0, 0, core, core, 10, 0, 0, caps_of(90))
    assert m["run_lengths"] == [89] and m["ops_by_step"] == 1
    # a lacks five bases behind its first: pos reaches 0 while x is 5, then five GAP_A steps in column pos == 0 and the last step, single ones
    ops = "M" + "A" * 5 + "M" * 84
    m = check(ops, 0, 0, core[:1] + core[6:], core, 10, 0, 0, caps_of(90))
    assert m["run_lengths"] == [84] and m["ops_by_step"] == 6
    # b's window begins 5 bases later: x reaches 0 while pos is 5
    ops = "M" * 85
    m = check(ops, 5, 5, core, core, 10, 0, 5, caps_of(85))
    assert m["run_lengths"] == [84] and m["ops_by_step"] == 1


def test_an_n_on_either_side_is_a_match():
    rng = random.Random(4)
    ops, a, b = diagonal_case(rng, 50, n_at_a=(0, 3, 16, 31), n_at_b=(3, 15, 32, 49), mism=(7,))
    m = check(ops, 0, 0, a, b, 20, 0, 0, caps_of(len(ops)), a_base=9, b_base=2)
    assert m["run_lengths"][0] == 50
    assert m["bytes"][:50].count(M.MISMATCH) == 1


def test_the_split_of_a_path_with_gaps():
    ops = "MMMMAMMBBMMXMMAAMMMM"
    by_run, by_step = M.split(ops, 2, 1, 0)
    assert by_run + by_step == len(ops) and by_step >= ops.count("A") + ops.count("B")
