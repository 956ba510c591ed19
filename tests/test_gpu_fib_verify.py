"""Verifying a batch of Fibonacci proofs on the device (include/toyni_hip.h 3t) through toyni_amd.verifier.verify_fib_batch.

The proofs come from the oracle-only prover (tests/harness/ref_prover.py): no device prover is involved.  Every row of the tamper matrix
(tests/fib_verify_cases.py) tampers the middle proof of a batch of three; the other two must still read 0, and the verdict -- name,
query, layer -- is held to tests/harness/fib_verifier.py on the same tampered proof.  n = 8 and 16 run the whole matrix, n = 256 (nine
folds, a final layer of sixteen) a batch of five with one row per verdict code.  A verdict does not depend on the batch it sits in,
batch 1 and batch 5 launch the same set of kernels, nothing outside the images' extent is read into a verdict and nothing outside
the outputs is written (guard bands), the refusals that need a real context come before anything is enqueued, and a captured graph
replays the chain on re-uploaded images."""
import ctypes

import numpy as np
import pytest

import fib_verify_cases as cases
from guarded import Guarded

pytestmark = pytest.mark.gpu
E_RANGE = 10006


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    if not toyni_amd.gpu_available():
        pytest.fail("no GPU visible")
    return toyni_amd


@pytest.fixture(scope="module")
def ctxs(ta):
    made = {}

    def get(n):
        if n not in made:
            made[n] = ta.NttContext(32 * n)
        return made[n]

    yield get
    for c in made.values():
        c.destroy()


def _swap_check(ta, raw, got, query, layer):
    # the one row where the position binding answers before the reference's check: same query, same layer
    assert cases.expected_of(raw) == (False, "fri_consistency") and got[1:] == ("fri_merkle", query, layer), got


@pytest.mark.parametrize("n", [8, 16])
def test_the_tamper_matrix_in_batches_of_three(ta, ctxs, n):
    valid = cases.proofs(n)
    ctx = ctxs(n)
    assert [v[0] for v in ta.verify_fib_batch(valid, ctx=ctx)] == [0, 0, 0]
    for label, fn, query, layer, fixed in cases.matrix(valid[1]):
        bad = cases.tampered(valid[1], fn)
        got = ta.verify_fib_batch([valid[0], bad, valid[2]], ctx=ctx)
        assert got[0][0] == 0 and got[2][0] == 0, (label, got)
        cases.check_verdict(label, got[1], bad, query, layer, fixed)
    fn, query, layer = cases.swap_row(valid[1])
    bad = cases.tampered(valid[1], fn)
    got = ta.verify_fib_batch([valid[0], bad, valid[2]], ctx=ctx)
    assert got[0][0] == 0 and got[2][0] == 0
    _swap_check(ta, bad, got[1], query, layer)


def test_one_row_per_code_at_nine_folds_in_a_batch_of_five(ta, ctxs):
    n = 256
    valid = cases.proofs(n)
    ctx = ctxs(n)
    rows = cases.matrix(valid[1], full=False)
    seen = set()
    for k in range(0, len(rows), 3):
        chunk = rows[k:k + 3]
        bads = [cases.tampered(valid[1], fn) for _, fn, _, _, _ in chunk]
        batch = [valid[0]] + bads + [valid[2]] * (4 - len(bads))
        got = ta.verify_fib_batch(batch, ctx=ctx)
        assert got[0][0] == 0 and all(g[0] == 0 for g in got[1 + len(bads):]), got
        for (label, _, query, layer, fixed), bad, g in zip(chunk, bads, got[1:]):
            cases.check_verdict(label, g, bad, query, layer, fixed)
            seen.add(g[1])
    assert seen == {"malformed", "ood", "final_not_constant", "final_commitment", "query_index", "trace_merkle", "quotient_merkle", "deep_merkle",
                    "deep_value", "fri_merkle", "fri_consistency", "final_value"}, seen


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import toyni_amd as ta
n, size = int(sys.argv[3]), int(sys.argv[4])
blob = open(sys.argv[2], "rb").read()
images = [blob[k:k + size] for k in range(0, len(blob), size)]
before = set(ta._lib.launched_kernels())
alone = [int(ta.verifier.verify_images([im], n)[0]) for im in images]
after_one = set(ta._lib.launched_kernels())
together = [int(w) for w in ta.verifier.verify_images(images, n)]
after_five = set(ta._lib.launched_kernels())
print(json.dumps({"before": sorted(before), "one": sorted(after_one), "five": sorted(after_five), "alone": alone, "together": together}))
"""


def test_a_verdict_does_not_depend_on_its_batch_and_both_batches_launch_the_same_kernels(ta, tmp_path):
    """In a FRESH process (the library's list of launched kernels is cumulative for a process): five proofs verified one by one, then
    the same five as one batch.  The verdicts are equal, the batches of one launched exactly the unit's five kernels (and nothing of
    them was launched before), and the batch of five launched no kernel that they had not."""
    import json
    import os
    import re
    import subprocess
    import sys
    import __graft_entry__ as entry
    n = 16
    valid = cases.proofs(n)
    rows = cases.matrix(valid[1], full=False)
    picks = [cases.tampered(valid[1], rows[k][1]) for k in (0, 9, 12, len(rows) - 4)] + [valid[0]]
    path = tmp_path / "images.bin"
    path.write_bytes(b"".join(ta.pack_fib_proof(p) for p in picks))
    res = subprocess.run([sys.executable, "-c", CHILD, entry.ROOT, str(path), str(n), str(ta.verifier.fib_proof_image_bytes(n))], capture_output=True, text=True,
                         timeout=120, env=dict(os.environ))
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    assert out["alone"] == out["together"] and out["together"][-1] == 0 and all(w != 0 for w in out["together"][:-1]), out
    assert out["together"] == [v[0] for v in ta.verify_fib_batch(picks)]
    unit = set(re.findall(r"Function Name: (\S+)", open(entry.RESOURCES_VERIFY).read()))
    before, one, five = set(out["before"]), set(out["one"]), set(out["five"])
    assert len(unit) == 5 and not unit & before
    assert unit <= one - before, sorted(unit - (one - before))   # the batches of one: all five kernels of the unit, none launched before
    assert five == one, sorted(five - one)                     # a batch of five: no kernel more


def test_guard_bands_stay_intact_and_nothing_outside_an_image_reaches_a_verdict(ta, ctxs):
    n, B = 8, 3
    lib = ta._lib.lib
    valid = cases.proofs(n)
    rows = cases.matrix(valid[1], full=False)
    raws = [valid[0], cases.tampered(valid[1], rows[12][1]), valid[2]]
    size = ta.verifier.fib_proof_image_bytes(n)
    stride = size + 48
    host = np.full(B * stride, 0xA5, dtype=np.uint8)
    for b, r in enumerate(raws):
        host[b * stride:b * stride + size] = np.frombuffer(ta.pack_fib_proof(r), dtype=np.uint8)
    images, work, out = (Guarded(ta, (B - 1) * stride + size, word=1, seed=1), Guarded(ta, lib.toyni_fib_verify_work_bytes(n, B), seed=2),
                         Guarded(ta, 4 * B, seed=3))
    try:
        want = [v[0] for v in ta.verify_fib_batch(raws, ctx=ctxs(n))]
        assert want[0] == 0 and want[1] != 0 and want[2] == 0
        for pattern in ("sentinel", "random"):
            images.refill(pattern)
            images.upload(host[:(B - 1) * stride + size])
            ta._lib.check(lib.toyni_fib_verify_batch_device(ctxs(n).handle, images.ptr, stride, n, B, work.ptr, out.ptr, None), "verify")
            ctxs(n).synchronize()
            assert out.download(np.uint32).tolist() == want, pattern
            for name, g in (("images", images), ("work", work), ("verdicts", out)):
                g.check(name)
            assert (images.download(np.uint8) == host[:(B - 1) * stride + size]).all()
        # the refusals behind the context's size, on a real context: outputs untouched
        out.fill_sentinel()
        work.fill_sentinel()
        h = ctxs(n).handle
        refused = {"another context": lib.toyni_fib_verify_batch_device(ctxs(16).handle, images.ptr, stride, n, B, work.ptr, out.ptr, None),
                   "images + 8": lib.toyni_fib_verify_batch_device(h, images.ptr + 8, stride, n, B, work.ptr, out.ptr, None),
                   "work + 4": lib.toyni_fib_verify_batch_device(h, images.ptr, stride, n, B, work.ptr + 4, out.ptr, None),
                   "verdicts + 2": lib.toyni_fib_verify_batch_device(h, images.ptr, stride, n, B, work.ptr, out.ptr + 2, None),
                   "stride short": lib.toyni_fib_verify_batch_device(h, images.ptr, size - 16, n, B, work.ptr, out.ptr, None),
                   "stride + 8": lib.toyni_fib_verify_batch_device(h, images.ptr, stride + 8, n, B, work.ptr, out.ptr, None)}
        assert all(rc == E_RANGE for rc in refused.values()), refused
        ctxs(n).synchronize()
        assert (out.download(np.uint8) == 0xA5).all() and (work.download(np.uint8) == 0xA5).all()
    finally:
        for g in (images, work, out):
            g.free()


def test_the_general_record_call_on_unsalted_trees_and_odd_leaf_counts(ta):
    """toyni_merkle_verify_records_batch_device on its own: two groups over trees the composite call never sees -- an unsalted tree and a
    tree of 5 leaves (an odd level pairs its last node with itself) -- against openings made and judged by the oracle."""
    import oracle
    from harness import ref_prover
    lib = ta._lib.lib
    B = 2
    rng = np.random.default_rng(7)
    groups, bufs, wants = [], [], []
    for leaves, salted in ((8, False), (5, True)):
        rb = ref_prover.merkle_record_bytes(leaves)
        idx = np.array([[0, leaves - 1, 2], [1, 3, leaves - 1]], dtype=np.uint32)
        recs, roots, want = np.zeros((B, 3 * rb), np.uint8), np.zeros((B, 32), np.uint8), np.ones((B, 3), np.uint32)
        for b in range(B):
            values = rng.integers(0, cases.P, leaves, dtype=np.uint64)
            salts = rng.integers(0, 256, (leaves, 16), dtype=np.uint8) if salted else None
            levels = oracle.merkle_commit_values(values, salts)
            _, raw = ref_prover.serialize_openings(levels, values, salts, idx[b])
            recs[b] = raw
            roots[b] = levels[-1][0]
        recs[1, rb + 3] ^= 1                      # proof 1, record 1: a path byte
        want[1, 1] = 0
        idx[0, 2] ^= 1                            # proof 0, record 2: the verifier expects its neighbour
        want[0, 2] = 0
        d = [Guarded(ta, a.nbytes, word=1, seed=len(bufs) + k) for k, a in enumerate((recs, idx, roots, want))]
        for g, a in zip(d[:3], (recs, idx, roots)):
            g.upload(a)
        bufs += d
        wants.append((d[3], want))
        groups.append(ta.verifier.MerkleVerifyGroup(d[0].ptr, 3 * rb, 3, leaves, int(salted), d[1].ptr, 3, d[2].ptr, 32, d[3].ptr, 3))
    try:
        arr = (ta.verifier.MerkleVerifyGroup * 2)(*groups)
        ta._lib.check(lib.toyni_merkle_verify_records_batch_device(arr, 2, B, None), "verify records")
        assert lib.toyni_stream_synchronize(None, None) == 0
        for g, want in wants:
            assert (g.download(np.uint32).reshape(B, 3) == want).all()
        for g in bufs:
            g.check("general call")
    finally:
        for g in bufs:
            g.free()


def test_a_captured_graph_replays_the_chain_on_re_uploaded_images(ta, ctxs):
    import torch
    n, B = 16, 3
    lib = ta._lib.lib
    dev = torch.device("cuda", 0)
    valid = cases.proofs(n)
    rows = cases.matrix(valid[1], full=False)
    size = ta.verifier.fib_proof_image_bytes(n)
    images = torch.zeros(B * size, dtype=torch.uint8, device=dev)
    work = torch.zeros(lib.toyni_fib_verify_work_bytes(n, B), dtype=torch.uint8, device=dev)
    out = torch.zeros(B, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    ctx = ctxs(n)

    def chain():
        ta._lib.check(lib.toyni_fib_verify_batch_device(ctx.handle, images.data_ptr(), size, n, B, work.data_ptr(), out.data_ptr(), s.cuda_stream), "verify")

    def load(raws):
        images.copy_(torch.from_numpy(np.frombuffer(b"".join(ta.pack_fib_proof(r) for r in raws), dtype=np.uint8).copy()).to(dev))
        work.fill_(0xA5)
        out.fill_(-1)
        torch.cuda.synchronize()

    load(valid)
    chain()                                              # eager first: the code objects are loaded
    ctx.synchronize(s.cuda_stream)
    assert out.cpu().numpy().view(np.uint32).tolist() == [0, 0, 0]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain()
    for picks in ((0, 12), (9, len(rows) - 4)):
        raws = [cases.tampered(valid[1], rows[picks[0]][1]), valid[0], cases.tampered(valid[1], rows[picks[1]][1])]
        want = [v[0] for v in ta.verify_fib_batch(raws, ctx=ctx)]
        assert want[0] != 0 and want[1] == 0 and want[2] != 0
        load(raws)
        g.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().view(np.uint32).tolist() == want
