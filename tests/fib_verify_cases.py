"""Proofs and the tamper matrix for the tests of include/toyni_hip.h 3t (a plain module, imported like tests/guarded.py).

The proofs come from the oracle-only prover (tests/harness/ref_prover.py) on an in-field Fibonacci column; no device code is involved
in making them.  A ROW of the matrix is (label, tamper, query, layer): `tamper(raw)` alters a copy of a proof in wire form in place;
the judge of what the verdict must be is tests/harness/fib_verifier.py on the expanded proof (`expected_of`), and (query, layer) is
what the row touched -- compared where the failing check belongs to a query / to a FRI layer.  Rows the Python verifier cannot express
(a word no BabyBear can hold) carry their expected verdict themselves."""
import copy
import os
import sys
from functools import lru_cache

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

P = 2013265921
Q = 44
PER_QUERY = ("query_index", "trace_merkle", "quotient_merkle", "deep_merkle", "deep_value", "fri_merkle", "fri_consistency", "final_value")


def trace_of(n, b):
    """An in-field Fibonacci column: a_0 = 1 + b, a_1 = 1."""
    out, a, c = [], 1 + b, 1
    for _ in range(n):
        out.append(a)
        a, c = c, (a + c) % P
    return np.array(out, dtype=np.uint64)


@lru_cache(maxsize=None)
def proofs(n, count=3):
    """`count` valid proofs of trace length n in wire form (computed once per session; callers copy before they tamper)."""
    from harness import ref_prover
    out = []
    for b in range(count):
        key = bytes((17 * b + 3 * i + n) & 0xFF for i in range(32))
        proof, _ = ref_prover.prove(trace_of(n, b), ref_prover.ChaChaRandomness(key))
        proof["opening_records"] = np.array(proof["opening_records"], dtype=np.uint8)
        out.append(proof)
    return tuple(out)


@lru_cache(maxsize=None)
def cheating_proof(n, kind, k=0):
    """A proof by a prover that CHEATS consistently, so that every Merkle check passes and a value check is the first to fail:
    kind "deep" commits and folds a DEEP layer that is one too large everywhere (DEEP_VALUE), kind "fold" adds one to every value of
    the layer after k folds (FRI_CONSISTENCY of layer k; k = the number of folds: FINAL_VALUE).  The oracle's functions are wrapped for
    the one call of ref_prover.prove and put back."""
    from harness import ref_prover
    orc = ref_prover.oracle
    deep0, fold0, calls = orc.fib_deep, orc.fri_fold, [0]

    def deep(*a, **kw):
        return (np.asarray(deep0(*a, **kw), dtype=np.uint64) + 1) % P

    def fold(*a, **kw):
        calls[0] += 1
        out = np.asarray(fold0(*a, **kw), dtype=np.uint64)
        return (out + 1) % P if calls[0] == k else out

    try:
        if kind == "deep":
            orc.fib_deep = deep
        else:
            orc.fri_fold = fold
        proof, _ = ref_prover.prove(trace_of(n, 5), ref_prover.ChaChaRandomness(bytes((29 * i + n + k) & 0xFF for i in range(32))))
    finally:
        orc.fib_deep, orc.fri_fold = deep0, fold0
    proof["opening_records"] = np.array(proof["opening_records"], dtype=np.uint8)
    return proof


def clone(raw):
    c = copy.deepcopy({k: v for k, v in raw.items() if k != "query_proofs"})
    c["opening_records"] = np.array(raw["opening_records"], dtype=np.uint8).copy()
    return c


def expected_of(raw):
    """(accepted, name) by the restated reference verifier."""
    from harness import fib_prover, fib_verifier
    why = []
    ok = fib_verifier.verify(fib_prover.expand_proof(raw), why)
    return ok, (why[0] if why else "accept")


# ---- where things lie in the serialized records ----
def record_bytes(leaves):
    d = leaves.bit_length() - 1
    return 32 * d + 24 + ((d + 7) & ~7)


def record_at(raw, group, j):
    """(byte offset of record j of group `group`, depth)"""
    off = 0
    for g, (tn, _s, idx) in enumerate(raw["opening_groups"]):
        if g == group:
            return off + j * record_bytes(tn), tn.bit_length() - 1
        off += len(idx) * record_bytes(tn)
    raise IndexError(group)


def folds_of(raw):
    return len(raw["fri_commitments"]) - 1


def _flip(raw, group, j, field, level=0):
    off, d = record_at(raw, group, j)
    r = raw["opening_records"]
    if field == "value":
        at = off + 32 * d + 16
        v = (int.from_bytes(r[at:at + 8].tobytes(), "little") + 1) % P
        r[at:at + 8] = np.frombuffer(v.to_bytes(8, "little"), dtype=np.uint8)
    elif field == "salt":
        r[off + 32 * d + 5] ^= 1
    elif field == "path":
        r[off + 32 * level + 7] ^= 0x10
    elif field == "position":
        r[off + 32 * d + 24 + level] ^= 1
    else:
        raise ValueError(field)


def _set_value_words(raw, group, j, lo, hi):
    off, d = record_at(raw, group, j)
    at = off + 32 * d + 16
    raw["opening_records"][at:at + 8] = np.frombuffer(int(lo).to_bytes(4, "little") + int(hi).to_bytes(4, "little"), dtype=np.uint8)


def _bit(raw, key, k=None):
    if k is None:
        b = bytearray(raw[key]); b[3] ^= 4; raw[key] = bytes(b)
    else:
        b = bytearray(raw[key][k]); b[3] ^= 4; raw[key][k] = bytes(b)


def _swap(raw, group, q):
    a, _ = record_at(raw, group, 2 * q)
    b, _ = record_at(raw, group, 2 * q + 1)
    n = b - a
    r = raw["opening_records"]
    tmp = r[a:a + n].copy()
    r[a:a + n] = r[b:b + n]
    r[b:b + n] = tmp


def matrix(raw, full=True):
    """The rows for a proof shaped like `raw`: (label, tamper, query, layer, fixed) -- tamper(copy) alters the copy in place (or returns
    the proof to take instead); fixed = None (ask the Python verifier) or the
    verdict name stated by the row itself."""
    F = folds_of(raw)
    fs = len(raw["fri_final_layer"])
    mid = (F + 1) // 2
    rows = []

    def row(label, fn, query=None, layer=None, fixed=None):
        rows.append((label, fn, query, layer, fixed))

    row("t_z + 1", lambda r: r.__setitem__("t_z", (r["t_z"] + 1) % P))
    row("q_z + 1", lambda r: r.__setitem__("q_z", (r["q_z"] + 1) % P))
    row("one final value + 1", lambda r: r["fri_final_layer"].__setitem__(fs - 1, (r["fri_final_layer"][fs - 1] + 1) % P), 0)
    row("every final value + 1", lambda r: r.__setitem__("fri_final_layer", [(v + 1) % P for v in r["fri_final_layer"]]), 0)
    row("trace root bit", lambda r: _bit(r, "trace_commitment"), 0)
    row("quotient root bit", lambda r: _bit(r, "quotient_commitment"), 0)
    row("fri_commitments[0] bit", lambda r: _bit(r, "fri_commitments", 0), 0)
    row("fri_commitments[mid] bit", lambda r: _bit(r, "fri_commitments", mid), 0)
    row("fri_commitments[last] bit", lambda r: _bit(r, "fri_commitments", F), 0)
    row("claimed query index", lambda r: r["query_indices"].__setitem__(5, r["query_indices"][5] ^ 1), 5)
    q = 7
    groups = [("trace row 0", 0, 3 * q, None), ("trace row 1", 0, 3 * q + 1, None), ("trace row 2", 0, 3 * q + 2, None), ("quotient", 1, q, None),
              ("DEEP", 2, 2 * q, None), ("DEEP pair", 2, 2 * q + 1, None), ("FRI layer 1", 3, 2 * q, 1), ("FRI layer %d" % mid, 2 + mid, 2 * q + 1, mid),
              ("FRI layer %d" % (F - 1), 2 + F - 1, 2 * q, F - 1)]
    for name, g, j, layer in groups:
        d = raw["opening_groups"][g][0].bit_length() - 1
        kinds = [("value", 0), ("salt", 0), ("path", 0), ("path", d - 1), ("position", 0)] if full else [("value", 0)]
        for field, level in kinds:
            row(f"{name}: {field}" + (f" level {level}" if field in ("path", "position") else ""),
                lambda r, g=g, j=j, field=field, level=level: _flip(r, g, j, field, level), q, layer)
    # two tamperings at once: the verdict is the earlier query's
    def both(r):
        _flip(r, 2 + mid, 2 * 30, "value")
        _flip(r, 1, 11, "path", 2)
    row("query 30 FRI value and query 11 quotient path", both, 11)
    row("quotient path in query 0", lambda r: _flip(r, 1, 0, "path", 1), 0)
    row("quotient path in query 43", lambda r: _flip(r, 1, 43, "path", 1), 43)
    # consistent cheating: every Merkle check passes, a value check is the first to fail (the row REPLACES the proof)
    n = int(raw["trace_len"])
    row("cheating prover: the DEEP layer + 1", lambda r: clone(cheating_proof(n, "deep")), 0)
    row("cheating prover: layer 1 + 1", lambda r: clone(cheating_proof(n, "fold", 1)), 0, 1)
    row("cheating prover: layer %d + 1" % (F - 1), lambda r: clone(cheating_proof(n, "fold", F - 1)), 0, F - 1)
    row("cheating prover: the final layer + 1", lambda r: clone(cheating_proof(n, "fold", F)), 0)
    # no Python counterpart: words no BabyBear can hold
    row("a trace value word >= p", lambda r: _set_value_words(r, 0, 3 * q, P, 0), None, None, "malformed")
    row("an upper value word != 0", lambda r: _set_value_words(r, 2 + mid, 2 * q, 5, 1), None, None, "malformed")
    row("t_gz = p", lambda r: r.__setitem__("t_gz", P), None, None, "malformed")
    return rows


def swap_row(raw):
    """op and op_pair swapped in one layer: (tamper, query, layer).  Both records still hash to the layer's root; the reference trusts
    their position flags and fails the layer's CONSISTENCY check, the device binds the flags to the derived positions and fails the
    layer's MERKLE check: same query, same layer, the check before."""
    mid = (folds_of(raw) + 1) // 2
    return (lambda r: _swap(r, 2 + mid, 9)), 9, mid


def tampered(raw, fn):
    r = clone(raw)
    out = fn(r)
    return r if out is None else out


def check_verdict(label, got, raw_tampered, query, layer, fixed):
    """got = (word, name, query, layer) of the device for the tampered proof."""
    word, name, gq, gl = got
    if fixed is not None:
        assert name == fixed and word != 0, (label, got)
        return
    ok, want = expected_of(raw_tampered)
    assert not ok, f"{label}: the Python verifier accepts this row"
    assert name == want, f"{label}: device {got}, Python verifier {want}"
    if want in PER_QUERY:
        assert gq == query, f"{label}: device {got}, the row touched query {query}"
    else:
        assert gq is None, (label, got)
    if want in ("fri_merkle", "fri_consistency"):
        assert layer is not None and gl == layer, f"{label}: device {got}, the row touched layer {layer}"


# ---- the word of every record, restated: leaf and path hash to the root AND the position bytes spell the DERIVED index ----
def derived_indices(raw):
    from harness import fib_verifier as fv
    N = int(raw["lde_size"])
    tr = fv.Transcript()
    tr.absorb(raw["trace_commitment"])
    tr.absorb(raw["quotient_commitment"])
    fv.derive_z(tr, N)
    for k in ("t_z", "t_gz", "t_ggz", "q_z"):
        tr.absorb(int(raw[k]).to_bytes(8, "little"))
    tr.absorb(raw["fri_commitments"][0])
    for c in raw["fri_commitments"][1:]:
        tr.squeeze_challenge()
        tr.absorb(c)
    return tr.squeeze_indices(Q, N // 2)


def expected_flags(raw):
    """One character per record, in the image's order."""
    from harness import fib_verifier as fv
    import toyni_amd
    N, F = int(raw["lde_size"]), folds_of(raw)
    qidx = derived_indices(raw)
    want = [[i for q in qidx for i in (q, (q + 32) % N, (q + 64) % N)], list(qidx), [i for q in qidx for i in (q, q + N // 2)]]
    cur = list(qidx)
    for k in range(1, F):
        half = (N >> k) // 2
        cur = [c % half for c in cur]
        want.append([i for c in cur for i in (c, c + half)])
    roots = [raw["trace_commitment"], raw["quotient_commitment"]] + list(raw["fri_commitments"])
    out, off = [], 0
    for g, (tn, salted, idx) in enumerate(raw["opening_groups"]):
        d, rb = tn.bit_length() - 1, record_bytes(tn)
        chunk = raw["opening_records"][off:off + rb * len(idx)]
        off += rb * len(idx)
        for j, op in enumerate(toyni_amd.prover.parse_openings(chunk, tn, want[g], salted)):
            pos_bytes = chunk[j * rb + 32 * d + 24:j * rb + 32 * d + 24 + d]
            spelled = all(int(pos_bytes[l]) == (want[g][j] >> l) & 1 for l in range(d))
            ok = op["value"] < P and spelled and fv.verify_opening(op, roots[g])
            out.append("1" if ok else "0")
    return "".join(out)
