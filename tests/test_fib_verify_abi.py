"""Verifying Fibonacci proofs on the device (include/toyni_hip.h 3t): the entry points are exported with the header's parameter counts
and bound in the Python package; every refusal the host decides before anything is enqueued comes from an otherwise valid call with
the outputs untouched, in the header's order (null pointers; batch; trace_len; the context's size -- held here on a block of stand-in
memory that no context of the right size can look like; the alignments and strides behind it need a real context and are held by
tests/test_gpu_fib_verify.py); the proof layout against its arithmetic restated here for every trace length; the packer's five
structural refusals under the reference's names; the names of the verdict words.  The pointers are host stand-in memory
(tests/guarded.py HostMem).  No compute."""
import ctypes
import os
import re

import numpy as np
import pytest

from guarded import Guarded, HostMem

E_INVALID_SIZE, E_NULL, E_RANGE = 10001, 10002, 10006
COUNTS = {"toyni_fib_proof_layout_of": 2, "toyni_fib_proof_image_bytes": 1, "toyni_fib_verdict_string": 1, "toyni_merkle_verify_records_batch_device": 4,
          "toyni_fib_verify_work_bytes": 2, "toyni_fib_verify_batch_device": 8}
Q, MASK = 44, 140


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def test_symbols_are_exported_and_bound_with_the_headers_parameter_counts(ta):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "toyni_hip.h")).read()
    assert header.index(" * 3s. ") < header.index(" * 3t. ") < header.index(" * 3c. ")
    for name, nargs in COUNTS.items():
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name), name
        f = getattr(ta._lib.lib, name)
        assert f.argtypes == ta._lib.SIGNATURES[name][1] and len(f.argtypes) == nargs
        decl = re.search(r"^(?:int|size_t|const char\*) %s\(([^;]*)\);" % name, header, re.M).group(1)   # the declaration, not a mention
        assert decl.count(",") + 1 == nargs, (name, decl)
    for name in ("pack_fib_proof", "verify_fib_batch"):
        assert hasattr(ta, name) and hasattr(ta.verifier, name)
    assert ctypes.sizeof(ta.verifier.FibProofLayout) == 8 * (12 + 4 * 32 + 2) and ctypes.sizeof(ta.verifier.MerkleVerifyGroup) == 88


def _record_bytes(leaves):
    d = leaves.bit_length() - 1
    return 32 * d + 24 + ((d + 7) & ~7)


def test_the_layout_is_its_arithmetic_for_every_trace_length(ta):
    lib = ta._lib.lib
    for log_n in range(3, 23):
        n = 1 << log_n
        lay = ta.verifier.fib_proof_layout(n)
        N = 32 * n
        C = 1 << (n + MASK - 1).bit_length()
        F, fs = C.bit_length() - 1, N // C
        assert (lay.trace_len, lay.lde_size, lay.folds, lay.final_size, lay.queries, lay.nroots, lay.ngroups) == (n, N, F, fs, Q, F + 3, F + 2)
        assert 1 <= fs <= 16 and F + 2 <= 32
        assert (lay.roots_offset, lay.ood_offset, lay.indices_offset, lay.final_offset) == (0, 32 * (F + 3), 32 * (F + 3) + 16, 32 * (F + 3) + 16 + 4 * Q)
        at = (lay.final_offset + 4 * fs + 7) & ~7
        assert lay.records_offset == at
        leaves = [N, N, N] + [N >> k for k in range(1, F)]
        counts = [3 * Q, Q, 2 * Q] + [2 * Q] * (F - 1)
        for g, (m, c) in enumerate(zip(leaves, counts)):
            assert (lay.group_offset[g], lay.group_leaves[g], lay.group_records[g], lay.group_record_bytes[g]) == (at, m, c, _record_bytes(m)), (n, g)
            assert lay.group_record_bytes[g] == lib.toyni_merkle_open_record_bytes(m) and at % 8 == 0
            at += c * _record_bytes(m)
        assert all(lay.group_records[g] == 0 for g in range(F + 2, 32))
        assert lay.nrecords == Q * (4 + 2 * F) == sum(counts)
        assert lay.image_bytes == (at + 15) & ~15 == lib.toyni_fib_proof_image_bytes(n)
        stride = (380 + 2 * lay.nrecords + 3) & ~3
        assert lib.toyni_fib_verify_work_bytes(n, 5) == 5 * 4 * stride
    lay = ta.verifier.FibProofLayout()
    for bad in (0, 4, 12, 1 << 23, (1 << 22) + 1):
        assert lib.toyni_fib_proof_layout_of(bad, ctypes.byref(lay)) == E_INVALID_SIZE and lib.toyni_fib_proof_image_bytes(bad) == 0
        assert lib.toyni_fib_verify_work_bytes(bad, 1) == 0
    assert lib.toyni_fib_proof_layout_of(8, None) == E_NULL
    assert lib.toyni_fib_verify_work_bytes(8, 0) == 0 and lib.toyni_fib_verify_work_bytes(8, 65536) == 0


def _untouched(buffers):
    for name, g in buffers:
        g.check(name)
        assert (g.download(np.uint8) == 0xA5).all(), name


def test_every_refusal_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    B, n = 3, 8
    size = lib.toyni_fib_proof_image_bytes(n)
    images, work, out, ctx, idx = (Guarded(mem, B * size, seed=1), Guarded(mem, lib.toyni_fib_verify_work_bytes(n, B), seed=2), Guarded(mem, 4 * B, seed=3),
                                   Guarded(mem, 1 << 16, seed=4), Guarded(mem, 4096, seed=5))
    try:
        def verify(c=ctx.ptr, im=images.ptr, st=size, tl=n, b=B, w=work.ptr, o=out.ptr):
            return lib.toyni_fib_verify_batch_device(c, im, st, tl, b, w, o, None)

        def group(**kw):
            g = ta.verifier.MerkleVerifyGroup(images.ptr, size, 4, 256, 1, idx.ptr, 4, images.ptr, size, out.ptr, 4)
            for k, v in kw.items():
                setattr(g, k, v)
            return g

        def records(g, b=B, count=1):
            return lib.toyni_merkle_verify_records_batch_device(ctypes.byref(g) if g is not None else None, count, b, None)

        nulls = {"ctx": verify(c=None), "images": verify(im=None), "work": verify(w=None), "verdicts": verify(o=None),
                 # a null pointer is named before a bad batch, a bad trace length and a bad stride
                 "images, batch 0": verify(im=None, b=0), "work, trace_len 12": verify(w=None, tl=12), "verdicts, stride 8": verify(o=None, st=8),
                 "groups": records(None), "records": records(group(d_records=None)), "indices": records(group(d_indices=None)),
                 "root": records(group(d_root=None)), "flags": records(group(d_flags=None)), "flags, batch 0": records(group(d_flags=None), b=0)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        ranges = {}
        for b in (0, 65536, 1 << 40):
            ranges[f"verify batch {b}"] = verify(b=b)
            ranges[f"records batch {b}"] = records(group(), b=b)
        # the batch is judged before the trace length (whose code differs), the trace length before the context
        sizes = {f"trace_len {tl}": verify(tl=tl) for tl in (0, 4, 12, 1 << 23)}
        assert verify(b=0, tl=12) == E_RANGE
        assert all(rc == E_INVALID_SIZE for rc in sizes.values()), sizes
        ranges.update({
            # the stand-in context is no context of 256 points: refused where the context is first read, before the alignments
            "context": verify(), "context, images + 8": verify(im=images.ptr + 8),
            "records + 4": records(group(d_records=images.ptr + 4)), "record stride + 4": records(group(record_stride=size + 4)),
            "record stride short": records(group(record_stride=4 * 288 - 8)), "leaves 0": records(group(leaves=0)),
            "leaves 2^32 + 1": records(group(leaves=(1 << 32) + 1, record_stride=1 << 20)), "records 2^26 + 1": records(group(nrecords=(1 << 26) + 1)),
            "indices + 2": records(group(d_indices=idx.ptr + 2)), "index stride 3": records(group(index_stride=3)), "root + 1": records(group(d_root=images.ptr + 1)),
            "root stride 16": records(group(root_stride=16)), "root stride 34": records(group(root_stride=34)), "flags + 2": records(group(d_flags=out.ptr + 2)),
            "flag stride 3": records(group(flag_stride=3))})
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # nothing to do: no groups, or groups without records -- whatever their other fields say
        assert records(None, count=0) == 0 and records(group(nrecords=0, d_records=None, leaves=0)) == 0
        _untouched([("images", images), ("work", work), ("verdicts", out), ("context", ctx), ("indices", idx)])
    finally:
        for g in (images, work, out, ctx, idx):
            g.free()


def test_the_packer_refuses_the_structure_the_reference_refuses_by_name(ta):
    import fib_verify_cases as cases
    v = ta.verifier
    good = cases.proofs(8)[0]
    assert len(v.pack_fib_proof(good)) == v.fib_proof_image_bytes(8)

    def refused(change):
        r = cases.clone(good)
        change(r)
        with pytest.raises(v.ProofStructureError) as e:
            v.pack_fib_proof(r)
        return e.value.name

    assert refused(lambda r: r.__setitem__("lde_size", 512)) == "lde_size"
    assert refused(lambda r: r["fri_commitments"].pop()) == "fold_count"
    assert refused(lambda r: r["fri_commitments"].append(bytes(32))) == "fold_count"
    assert refused(lambda r: r.__setitem__("fri_commitments", [])) == "fold_count"
    assert refused(lambda r: r["fri_final_layer"].append(1)) == "final_size"
    assert refused(lambda r: r.__setitem__("fri_final_layer", [])) == "final_size"
    assert refused(lambda r: r["query_indices"].pop()) == "query_count"
    assert refused(lambda r: r.__setitem__("opening_records", r["opening_records"][:-8])) == "fri_opening_count"
    assert refused(lambda r: r.__setitem__("opening_records", np.concatenate([r["opening_records"], np.zeros(8, np.uint8)]))) == "fri_opening_count"
    assert refused(lambda r: r.__setitem__("opening_records", np.zeros(0, np.uint8))) == "fri_opening_count"
    # the restated reference verifier gives the same names where its proof structure can carry the defect
    from harness import fib_prover, fib_verifier
    for change, name in ((lambda p: p.__setitem__("lde_size", 512), "lde_size"), (lambda p: p["fri_commitments"].pop(), "fold_count"),
                         (lambda p: p["fri_final_layer"].append(1), "final_size"), (lambda p: p["query_proofs"].pop(), "query_count"),
                         (lambda p: p["query_proofs"][3]["fri_openings"].pop(), "fri_opening_count")):
        p = fib_prover.expand_proof(cases.clone(good))
        change(p)
        why = []
        assert not fib_verifier.verify(p, why) and why == [name]


def test_every_verdict_word_has_its_name(ta):
    v = ta.verifier
    names = {0: "accept", 1: "malformed", 2: "ood", 3: "final_not_constant", 4: "final_commitment"}
    for word, name in names.items():
        assert v.decode_verdict(word) == (word, name, None, None)
    per_query = {5: "query_index", 6: "trace_merkle", 7: "quotient_merkle", 8: "deep_merkle", 9: "deep_value", 255: "final_value"}
    for q in (0, 43):
        for code, name in per_query.items():
            assert v.decode_verdict((q + 1) << 8 | code) == ((q + 1) << 8 | code, name, q, None)
        for k in range(1, 23):
            assert v.decode_verdict((q + 1) << 8 | (16 + 2 * (k - 1)))[1:] == ("fri_merkle", q, k)
            assert v.decode_verdict((q + 1) << 8 | (17 + 2 * (k - 1)))[1:] == ("fri_consistency", q, k)
    for word in (5, 9, 255, 1 << 8 | 1, 1 << 8 | 4, 1 << 8 | 10, 45 << 8 | 5, 1 << 8 | 200):
        assert v.verdict_string(word) == "unknown", word


def test_the_stored_proof_image_of_the_smoke_run_is_the_oracle_only_provers(ta):
    """tests/golden/fib_verify/proof_n8.image, which __graft_entry__.smoke() verifies: the packed proof of tests/harness/ref_prover.py for the
    column 1, 1, 2, 3, ... of 8 rows under the key 00 .. 1f, accepted by the restated reference verifier."""
    import fib_verify_cases as cases
    from harness import ref_prover
    proof, _ = ref_prover.prove(cases.trace_of(8, 0), ref_prover.ChaChaRandomness(bytes(range(32))))
    assert cases.expected_of(proof) == (True, "accept")
    stored = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fib_verify", "proof_n8.image"), "rb").read()
    assert stored == ta.pack_fib_proof(proof)
