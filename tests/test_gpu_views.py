"""Sequence views (gamdp_task a_rc / b_rc / a_off / b_off: reverse complement first, then the suffix) through every alignment kernel.

The contract (include/gamdp.h): a view gives exactly what an explicitly reverse-complemented / chopped copy gives.  The cases of
tests/_views.py hold, per side, a stored sequence, a view spec and the copy; truth is the oracle on the copies, which knows nothing of
views.  For each kernel of kernel_info (gamdp_kernel.hip) one batched gamdp_align_batch call holds, for every case, the view call AND
the copy call: view == copy == oracle on key() and on the edit string, and the library's own account of the call (gamdp_ctx_launch_info)
must name the kernel the cell was built for -- a planner change that routes the cases elsewhere fails the test instead of hollowing it out.
The cells a small batch reaches only through a planner switch (GAMDP_QUAD_MIN, GAMDP_NO_PAIR: read once per process) run in fresh child
processes, each under its own timeout.

Nothing here is built to fault: every input is a valid call, or one the library documents that it refuses on the host before any launch.
"""
import ctypes as C
import json
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import _mixed
import _oracle as O
import _views as V
from _gpu import ctx
import gam_ngs_amd as gam
from gam_ngs_amd import api
from gam_ngs_amd import lib as L

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEEN = {}          # cell -> kernel names the view cases of that cell ran on (this process and the children)
_CASES = {}


def _cases(group):
    if group not in _CASES:
        _CASES[group] = V.matrix_cases() if group == "main" else V.nbait_cases()
    return _CASES[group]


def _oracle_all(cases):
    def one(c):
        o, ops = O.oracle_align(c["a"], c["b"], c["band"], c["begin_a"], c["end_a"], c["begin_b"], c["end_b"], c["fs"], c["fe"], want_ops=True)
        return o.key(), ops
    with ThreadPoolExecutor(16) as ex:   # (the oracle's C code runs outside the GIL)
        return list(ex.map(one, cases))


def run_view_and_copy(c, cases, want_ops=True, bsw_ctx=None, set_cls=gam.SequenceSet):
    """One batched call: for every case the view call on the stored sequences, then the copy call.  -> [(view result, copy result)]"""
    seqs = []
    for cs in cases:
        seqs += [cs["stored_a"], cs["stored_b"], cs["a"], cs["b"]]
    sset = set_cls(c, seqs, ascii=False)
    calls, bands = [], []
    for i, cs in enumerate(cases):
        w = (cs["begin_a"], cs["end_a"])
        calls.append((sset.contig(4 * i, *cs["va"]), w[0], w[1], sset.contig(4 * i + 1, *cs["vb"]), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
        calls.append((sset.contig(4 * i + 2), w[0], w[1], sset.contig(4 * i + 3), cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
        bands += [cs["band"], cs["band"]]
    res = gam.BandedSmithWaterman(bsw_ctx or c).find_alignments(calls, want_ops=want_ops, bands=bands)
    sset.close()
    return [(res[2 * i], res[2 * i + 1]) for i in range(len(cases))]


def compare(cases, res, want, with_ops, dg):
    """view == copy == oracle; every case is compared, whatever its status.  -> number of cases with an alignment"""
    bad = []
    for cs, (rv, rc_), (okey, oops) in zip(cases, res, want):
        if rv.key() != okey or rc_.key() != okey or (with_ops and (rv.ops != oops or rc_.ops != oops)):
            bad.append(dict(tag=cs["tag"], view=rv.key(), copy=rc_.key(), oracle=okey,
                            ops_differ=(with_ops and (rv.ops != oops, rc_.ops != oops))))
    assert not bad, ("digest " + dg, len(bad), bad[:3])
    return sum(1 for k, _ in want if k[0] == O.OK and k[5] > 0)


def check_cell(cell):
    """The main batch of a cell, with and without edit strings, and (for the N-free tuned kernels) its two N-bait batches."""
    c = ctx()
    name, bands, n_mode, env = V.CELLS[cell]
    for k, v in env.items():
        assert os.environ.get(k) == v, "cell %s needs %s=%s in the process's environment (a fresh child)" % (cell, k, v)
    cases = [cs for cs in _cases("main") if cs["cell"] == cell]
    dg = V.digest(_cases("main"))
    want = _oracle_all(cases)
    names = set()
    for with_ops in (True, False):
        res = run_view_and_copy(c, cases, want_ops=with_ops)
        info = c.launch_info()
        n_ok = compare(cases, res, want, with_ops, dg)
        assert n_ok >= 0.9 * len(cases), (cell, n_ok, len(cases))
        # the kernel the cell was built for ran, and nothing else did
        assert {r["kernel"] for r in info} == {name}, (cell, dg, info)
        assert sum(r["tasks"] for r in info) == 2 * len(cases), (cell, info)
        if n_mode:   # every window holds an N: never an N-free kernel
            assert all(r["n_aware"] for r in info), (cell, info)
        names |= {r["kernel"] for r in info}
    SEEN[cell] = sorted(names)
    nb = [cs for cs in _cases("nbait") if cs["cell"] == cell]
    if not nb:
        return
    # N by window on views: the N lies in the chopped-off prefix, `dist` bases in front of the view -- outside every window (truth: no N),
    # inside or outside the 256-base blocks the library decides by.  Predicted with the Python mirror of npre_window_has_n
    # (tests/test_views_cpu.py checks both against brute force).
    dgn = V.digest(_cases("nbait"))
    assert all(V.window_truth_n(cs) is False for cs in nb)
    pred = [V.call_block_answer(cs) for cs in nb]
    assert any(pred) and not all(pred), (cell, "the N bait must fall on both sides of the library's choice", pred)
    for flag in (False, True):
        part = [cs for cs, p in zip(nb, pred) if p == flag]
        res = run_view_and_copy(c, part, want_ops=True)
        info = c.launch_info()
        compare(part, res, _oracle_all(part), True, dgn)
        if not flag:    # no N within the blocks any call touches: the N-free kernel alone
            assert {r["kernel"] for r in info} == {name} and not any(r["n_aware"] for r in info), (cell, dgn, info, [cs["tag"] for cs in part][:2])
        else:           # the view calls are N-aware by the block answer (accepted: conservative), their copies hold no N at all
            assert any(r["n_aware"] for r in info), (cell, dgn, info)
            assert sum(r["tasks"] for r in info if r["n_aware"]) >= len(part), (cell, info)


def _env_key(env):
    return tuple(sorted(env.items()))


def cells_for(env):
    return [k for k, v in V.CELLS.items() if _env_key(v[3]) == _env_key(env)]


def child_main():
    """Inside a fresh child process: the cells that need this process's planner switches."""
    env = {k: os.environ[k] for k in ("GAMDP_QUAD_MIN", "GAMDP_NO_PAIR") if k in os.environ}
    for cell in cells_for(env):
        check_cell(cell)
    print("VIEW_KERNELS " + json.dumps(SEEN))


def run_child(env):
    """A fresh child (never exec) with the planner switches of `env`, under its own timeout."""
    if all(c in SEEN for c in cells_for(env)):
        return
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_views as T\nT.child_main()\n") % (os.path.dirname(HERE), HERE)
    full = {k: v for k, v in os.environ.items() if k not in ("GAMDP_QUAD_MIN", "GAMDP_NO_PAIR", "GAMDP_NO_MERGE_N")}
    full.update(env)
    r = subprocess.run([sys.executable, "-c", code], env=full, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (env, r.stdout[-3000:] + r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("VIEW_KERNELS ")]
    assert line, r.stdout[-2000:]
    SEEN.update(json.loads(line[-1][len("VIEW_KERNELS "):]))


DEFAULT_CELLS = cells_for({})
CHILD_ENVS = sorted({_env_key(v[3]) for v in V.CELLS.values() if v[3]})


@pytest.mark.parametrize("cell", DEFAULT_CELLS)
def test_views_equal_copies_equal_oracle(cell):
    check_cell(cell)


@pytest.mark.parametrize("env", CHILD_ENVS, ids=lambda e: "+".join("%s=%s" % kv for kv in e))
def test_views_equal_copies_equal_oracle_in_a_fresh_process(env):
    run_child(dict(env))


def test_degenerate_views():
    """off == len (an empty view), off == len - 1, off > len (status INVALID, the rest of the batch still correct), rc of sequences of
    length 1 and 0: the view call gives what the oracle gives on the copy; where no copy exists the status is INVALID."""
    c = ctx()
    cases = V.degenerate_cases()
    seqs, calls, bands, want, wops = [], [], [], [], []
    for i, cs in enumerate(cases):
        a, b = V.apply_view(cs["stored_a"], *cs["va"]), V.apply_view(cs["stored_b"], *cs["vb"])
        seqs += [cs["stored_a"], cs["stored_b"]]
        want.append(None if a is None or b is None else
                    O.oracle_align(a, b, cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"]))
        wops.append(want[-1] is not None)
    sset = gam.SequenceSet(c, seqs, ascii=False)
    for i, cs in enumerate(cases):
        calls.append((sset.contig(2 * i, *cs["va"]), cs["begin_a"], cs["end_a"], sset.contig(2 * i + 1, *cs["vb"]), cs["begin_b"], cs["end_b"],
                      cs["fs"], cs["fe"]))
        bands.append(cs["band"])
    res = gam.BandedSmithWaterman(c).find_alignments(calls, want_ops=wops, bands=bands)
    seen = {}
    for cs, r, w in zip(cases, res, want):
        if w is None:
            assert r.status == L.ST_INVALID and r.cells == 0, (cs["tag"], r.key())
        elif w[0].status == O.INVALID:
            assert r.status == O.INVALID, (cs["tag"], r.key())
        else:
            assert r.key() == w[0].key() and r.ops == w[1], (cs["tag"], r.key(), w[0].key())
        seen[r.status] = seen.get(r.status, 0) + 1
    assert seen.get(L.ST_OK, 0) >= 20 and seen.get(L.ST_INVALID, 0) >= 36, seen
    sset.close()


def test_driver_shaped_batch_with_views_on_both_sides():
    """tests/_mixed.py's driver-shaped batch (16 384 band-150 calls: chain calls, left tails, right tails on chop_begin views) with 40 % of
    the contigs stored reverse-complemented, behind a chopped-off prefix, or both: b_off != 0, b_rc, a_rc and rc + off, unequal
    b_base among the tasks of a wavefront of the packed kernels.  Through the planner's own choice, against the oracle on the plain batch."""
    from test_gpu_mixed_batch import oracle_keys, run_batch
    c = ctx()
    stored, calls, plain = _mixed.mixed_batch(20261004, 2048, 8, views=0.4)
    assert len(calls) == 16384
    plain_calls = [dict(cl, a_off=cl["a_off"] - (len(stored[cl["a_id"]]) - len(plain[cl["a_id"]]))) for cl in calls]
    for cl, pc in zip(calls[:400], plain_calls[:400]):   # the views of the stored contigs are the plain contigs
        assert V.apply_view(stored[cl["a_id"]], cl["a_rc"], cl["a_off"]) == plain[cl["a_id"]][pc["a_off"]:]
        assert V.apply_view(stored[cl["b_id"]], cl["b_rc"], cl["b_off"]) == plain[cl["b_id"]]
    sset = gam.SequenceSet(c, stored, ascii=False)
    out = run_batch(c, sset, calls)
    info = c.launch_info()
    want = oracle_keys(plain, plain_calls)
    bad = [i for i in range(len(calls)) if tuple(out[i].key()) != tuple(want[i])]
    assert not bad, (len(bad), calls[bad[0]], out[bad[0]].key(), want[bad[0]])
    n = len(calls)
    assert sum(1 for cl in calls if cl["b_off"]) > 0.15 * n and sum(1 for cl in calls if cl["b_rc"]) > 0.15 * n
    assert sum(1 for cl in calls if cl["a_rc"]) > 0.15 * n and sum(1 for cl in calls if cl["a_rc"] and cl["a_off"]) > 0.08 * n
    assert sum(1 for cl in calls if cl["b_rc"] and cl["b_off"]) > 0.08 * n
    assert sum(1 for k in want if k[0] == O.OK) > 15000
    assert "k_align_o<19,15>" in {r["kernel"] for r in info} and any(r["n_aware"] for r in info), info
    sset.close()


def _lifecycle_set(rng, n_pairs=20):
    """Contigs 2k / 2k+1 with contig 2k+1 a diverged copy of the REVERSE COMPLEMENT of contig 2k: the rc view of either aligns with the other."""
    seqs = []
    for k in range(n_pairs):
        a = bytearray(V.rand_codes(rng, rng.choice((200, 700, 1500, 3000))))
        if k % 5 == 0:
            p = rng.randrange(len(a) - 10)
            a[p:p + 4] = b"\4\4\4\4"
        seqs += [bytes(a), V.mutate(rng, V.revcomp(bytes(a)))]
    return seqs


def test_the_lazy_reverse_complement_planes_over_several_batches_and_two_contexts():
    """SeqSet::ensure_rc packs and uploads the rc copy of a contig the first time a batch asks for it, into a fresh allocation per
    batch.  Batch 1 asks for rc of ids {0, 3}, batch 2 for {3, 4, 5, 0} (cached and new ids mixed, several new ones at once), batch 3 for
    all, on a second context on the same device while the first is alive, batch 4 repeats batch 1.  Every result equals that of the
    same call on a fresh set of explicit copies, and the oracle's."""
    rng = random.Random(20261017)
    seqs = _lifecycle_set(rng)
    n = len(seqs)
    c1 = ctx()
    c2 = gam.Context(0)
    sset = gam.SequenceSet(c1, seqs, ascii=False)
    copies = gam.SequenceSet(c1, seqs + [V.revcomp(s) for s in seqs], ascii=False)

    def calls_for(ids, on, rc_views):
        out = []
        for i in ids:
            a, b = (i, i + 1) if i % 2 == 0 else (i - 1, i)    # the pair of contig i; contig i is the reverse-complemented one
            if rc_views:
                A, B = on.contig(a, rc=(a == i)), on.contig(b, rc=(b == i))
            else:
                A, B = on.contig(a + n if a == i else a), on.contig(b + n if b == i else b)
            out.append((A, 0, len(seqs[a]) - 1, B, 0, len(seqs[b]) - 1))
        return out

    for bno, (ids, c) in enumerate((([0, 3], c1), ([3, 4, 5, 0], c1), (list(range(n)), c2), ([0, 3], c1))):
        got = gam.BandedSmithWaterman(c, 150).find_alignments(calls_for(ids, sset, True), want_ops=True)
        ref = gam.BandedSmithWaterman(c1, 150).find_alignments(calls_for(ids, copies, False), want_ops=True)
        for i, g, r in zip(ids, got, ref):
            a, b = (i, i + 1) if i % 2 == 0 else (i - 1, i)
            sa, sb = (V.revcomp(seqs[a]) if a == i else seqs[a]), (V.revcomp(seqs[b]) if b == i else seqs[b])
            o, ops = O.oracle_align(sa, sb, 150, 0, len(sa) - 1, 0, len(sb) - 1)
            assert g.key() == r.key() == o.key() and g.ops == r.ops == ops, ("batch", bno + 1, "rc of contig", i, g.key(), r.key(), o.key())
            assert o.status == O.OK and o.length > 100, (bno, i)
    # forward views of the same set are untouched by all that
    fw = gam.BandedSmithWaterman(c1, 150).find_alignments([(sset.contig(2), 0, len(seqs[2]) - 1, sset.contig(2), 0, len(seqs[2]) - 1)])
    assert fw[0].status == O.OK and fw[0].length() == len(seqs[2]) and 4 not in seqs[2]
    sset.close(); copies.close(); c2.close()


def test_rc_view_of_an_ascii_set_with_lower_case_and_iupac_letters():
    """A set uploaded as ASCII: lower case maps to the base, every other letter to N (tests/golden/seqops.json pins the rules); its rc view
    must be encode(revcomp) under those rules."""
    rng = random.Random(3)
    core = "".join(rng.choice("ACGTacgt") for _ in range(1200))
    a = core[:300] + "RYKMxX-*nN" + core[300:700] + "n" + core[700:]
    b_codes = V.mutate(rng, V.revcomp(O.encode(a)))
    b = "".join("ATCGN"[x] if rng.random() < 0.5 else "atcgn"[x] for x in b_codes)
    assert api.encode(a) == O.encode(a) and api.encode(b) == b_codes
    assert O.encode("acgtnACGTNRYKMxX-*") == bytes([0, 2, 3, 1, 4, 0, 2, 3, 1, 4, 4, 4, 4, 4, 4, 4, 4, 4])
    c = ctx()
    sset = gam.SequenceSet(c, [a.encode(), b.encode()], ascii=True)
    bsw = gam.BandedSmithWaterman(c, 150)
    for off_a, off_b in ((0, 0), (17, 33)):
        ra = V.revcomp(O.encode(a))[off_a:]
        r = bsw.find_alignment(sset.contig(0, rc=True, off=off_a), 0, len(ra) - 1, sset.contig(1, off=off_b), 0, len(b) - off_b - 1, want_ops=True)
        o, ops = O.oracle_align(ra, b_codes[off_b:], 150, 0, len(ra) - 1, 0, len(b) - off_b - 1)
        assert r.key() == o.key() and r.ops == ops and o.length > 1000, (off_a, off_b, r.key(), o.key())
        rb = V.revcomp(b_codes)[off_b:]
        r = bsw.find_alignment(sset.contig(0, off=off_a), 0, len(a) - off_a - 1, sset.contig(1, rc=True, off=off_b), 0, len(rb) - 1, want_ops=True)
        o, ops = O.oracle_align(O.encode(a)[off_a:], rb, 150, 0, len(a) - off_a - 1, 0, len(rb) - 1)
        assert r.key() == o.key() and r.ops == ops, (off_a, off_b, r.key(), o.key())
    sset.close()


def test_all_sixteen_view_kinds_through_the_multi_layer():
    """The band-150 cells (N-free and with N) through gamdp_multi_align_batch on two contexts on device 0 (what tests/test_gpu_multi.py
    builds): view == copy == oracle."""
    cases = [cs for cs in _cases("main") if cs["cell"] in ("c5", "c5n") and not cs["tag"].get("long")]
    assert {cs["tag"]["kinds"] for cs in cases} == set(V.KIND_PAIRS)
    m = gam.MultiContext([0, 0])
    res = run_view_and_copy(m, cases, want_ops=False, set_cls=gam.MultiSequenceSet)
    compare(cases, res, _oracle_all(cases), False, V.digest(_cases("main")))
    m.close()


def _good_call_follows(c, what):
    """The context is usable after a refusal: a correct call, compared with the oracle."""
    cs = [x for x in _cases("main") if x["cell"] == "c5n"][5]
    (rv, rc_), = run_view_and_copy(c, [cs], want_ops=True)
    o, ops = O.oracle_align(cs["a"], cs["b"], cs["band"], cs["begin_a"], cs["end_a"], cs["begin_b"], cs["end_b"], cs["fs"], cs["fe"])
    assert rv.key() == rc_.key() == o.key() and rv.ops == ops and o.status == O.OK, ("after " + what, rv.key(), o.key())


def test_refusals_leave_the_context_usable():
    """What the library refuses on the host before any launch: ids out of range (GAMDP_EINVAL, "sequence id out of range"), rc on a
    packed-only (synthetic) set inside a large batch (the first offender by index decides the message), NULL set / NULL out; and
    off > len, which is no refusal but a per-task status.  A correct call follows each."""
    c = ctx()
    lib = c.lib
    rng = random.Random(9)
    seqs = [V.rand_codes(rng, 500) for _ in range(4)]
    sset = gam.SequenceSet(c, seqs, ascii=False)

    def batch(n, edit):
        tasks = (L.Task * n)()
        for k, t in enumerate(tasks):
            t.a_id, t.b_id, t.band = k % 4, (k + 1) % 4, 150
            t.begin_a, t.end_a, t.begin_b, t.end_b = 0, 499, 0, 499
        edit(tasks)
        return tasks, (L.Result * n)()

    for which in ("a_id", "b_id"):
        for bad_id in (4, 2 ** 32 - 1):
            tasks, out = batch(10, lambda ts: setattr(ts[7], which, bad_id))
            assert lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, 10, out, None) == L.EINVAL
            assert "sequence id out of range" in c.last_error()
            _good_call_follows(c, "%s = %d" % (which, bad_id))
    # rc on a synthetic set, inside a batch of 20 000 (checked on the host pool's threads): task 12 345 is the first offender, a band
    # beyond GAMDP_MAX_BAND comes later -- the message is the first offender's
    synth = gam.SequenceSet.synthetic(c, 5, 4, 300)
    n = 20000

    def edit(ts):
        for t in ts:
            t.a_id, t.b_id, t.end_a, t.end_b = 0, 1, 299, 299
        ts[12345].b_rc = 1
        ts[15000].a_rc = 1
        ts[17000].band = (1 << 20) + 1
    tasks, out = batch(n, edit)
    assert lib.gamdp_align_batch(c.handle, synth.handle, synth.handle, tasks, n, out, None) == L.EINVAL
    assert "reverse complement requested on a packed-only" in c.last_error()
    tasks[12000].band = (1 << 20) + 1          # now the band is the first offender
    assert lib.gamdp_align_batch(c.handle, synth.handle, synth.handle, tasks, n, out, None) == L.ENOTSUP
    assert "GAMDP_MAX_BAND" in c.last_error()
    _good_call_follows(c, "rc on a synthetic set")
    synth.close()
    # off > len: INVALID for that task, the rest of the batch correct
    tasks, out = batch(12, lambda ts: (setattr(ts[3], "a_off", 501), setattr(ts[8], "b_off", 1 << 33), setattr(ts[9], "b_off", 500)))
    assert lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, 12, out, None) == 0, c.last_error()
    for k in range(12):
        if k in (3, 8):
            assert out[k].status == L.ST_INVALID, k
            continue
        b = seqs[(k + 1) % 4][500 if k == 9 else 0:]
        o, _ = O.oracle_align(seqs[k % 4], b, 150, 0, 499, 0, 499, want_ops=False)
        assert tuple(out[k].key()) == tuple(o.key()), (k, out[k].key(), o.key())
    # NULL set / NULL out
    tasks, out = batch(4, lambda ts: None)
    assert lib.gamdp_align_batch(c.handle, None, sset.handle, tasks, 4, out, None) == L.EINVAL
    _good_call_follows(c, "NULL set a")
    assert lib.gamdp_align_batch(c.handle, sset.handle, None, tasks, 4, out, None) == L.EINVAL
    assert lib.gamdp_align_batch(c.handle, sset.handle, sset.handle, tasks, 4, None, None) == L.EINVAL
    _good_call_follows(c, "NULL out")
    sset.close()


def test_zz_every_kernel_of_kernel_info_ran_on_view_cases():
    """After the whole module: the union of the kernel names the view cases ran on equals the names in kernel_info.  (Cells that a
    selection of tests left out are run here.)"""
    for cell in DEFAULT_CELLS:
        if cell not in SEEN:
            check_cell(cell)
    for env in CHILD_ENVS:
        run_child(dict(env))
    assert set(SEEN) == set(V.CELLS)
    ran = {k for names in SEEN.values() for k in names}
    assert ran == V.kernel_names_in_source(), (sorted(ran), sorted(V.kernel_names_in_source()))
