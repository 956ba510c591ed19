"""The four-to-one Ext FRI calls under coset leaves (include/toyni_hip.h 3m): exported with the header's parameter counts, bound in the
Python package, and every refusal of the header that the arguments alone decide, from an otherwise valid call with the outputs
untouched.  Those refusals come before the context is read and before anything is enqueued, so they can be asked for without a
device: the pointers are host stand-in memory (tests/guarded.py HostMem), the context a block of it that a call which passed its
checks would misread -- none does.  "m exceeds the context's n" needs a real context and belongs to
tests/test_gpu_fold4_commit_ext.py.  No compute (no GPU here)."""
import ctypes
import os

import numpy as np
import pytest

from guarded import Guarded, HostMem, P

E_INVALID_SIZE, E_NULL, E_ZERO_INVERSE, E_RANGE = 10001, 10002, 10005, 10006

COUNTS = {"toyni_merkle_commit_cosets_ext_device": 5, "toyni_merkle_open_cosets_ext_device": 8, "toyni_fri_fold4_commit_ext_device": 9,
          "toyni_fri4_query_positions_device": 6, "toyni_fri4_commit_phase_transcript_ext_device": 11}


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def untouched(*named):
    for name, g in named:
        g.check(name)
        assert (g.download(np.uint8) == 0xA5).all(), name


def test_symbols_are_exported_and_bound_with_the_headers_parameter_counts(ta):
    for name, nargs in COUNTS.items():
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name)
        f = getattr(ta._lib.lib, name)
        assert f.argtypes == ta._lib.SIGNATURES[name][1] and len(f.argtypes) == nargs and f.restype is ctypes.c_int
    # the same shapes as the two-to-one calls they stand beside
    sig = ta._lib.SIGNATURES
    assert sig["toyni_fri_fold4_commit_ext_device"][1] == sig["toyni_fri_fold_commit_ext_device"][1]
    assert sig["toyni_fri4_commit_phase_transcript_ext_device"][1] == sig["toyni_fri_commit_phase_transcript_ext_device"][1]
    assert sig["toyni_fri4_query_positions_device"][1] == sig["toyni_fri_query_positions_device"][1]
    for name in ("fri_fold4_commit_ext_device", "fri4_query_positions_device", "fri4_commit_phase_transcript_ext_device"):
        assert hasattr(ta.prover, name)
    for name in ("CosetExtMerkleTree", "merkle_commit_cosets_ext_device", "merkle_open_cosets_ext_device"):
        assert hasattr(ta, name) and hasattr(ta.merkle, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "toyni_hip.h")).read()
    for name, nargs in COUNTS.items():
        decl = header.split("int " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == nargs, (name, decl)
    # the public layout constants of 3d are what they were: the coset layout is internal
    assert "#define TOYNI_ROWS_COLUMN_MAJOR 0" in header and "#define TOYNI_ROWS_ROW_MAJOR 1" in header and "TOYNI_ROWS_EXT" not in header


def test_the_hashlib_coset_tree_is_the_row_tree_of_the_gathered_layer(ta):
    import rows_common as rc
    rng = np.random.default_rng(5)
    for m in (4, 16, 64):
        layer = rng.integers(0, P, (m, 4), dtype=np.uint64)
        salts = rng.integers(0, 256, (m // 4, 16), dtype=np.uint8)
        rows = np.stack([np.concatenate([layer[j + s * (m // 4)] for s in range(4)]) for j in range(m // 4)])
        assert (ta.merkle.coset_rows(layer) == rows).all()
        for s in (salts, None):
            tree = ta.CosetExtMerkleTree(layer, s)
            want = rc.hashlib_levels(rc.leaves_of(rows, s))
            assert tree.levels == want and tree.root() == want[-1][0] and tree.n == m // 4
            assert tree.flat().tobytes() == b"".join(d for level in want for d in level)
            assert tree.leaf_bytes(m // 4 - 1) == rc.leaves_of(rows, s)[-1]


def test_every_refusal_of_the_round_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    m = 64
    evals, out, salts = Guarded(mem, 16 * m, seed=1), Guarded(mem, 4 * m, seed=2), Guarded(mem, 16 * (m // 16), seed=3)
    levels, fake_ctx = Guarded(mem, 32 * 7, word=1, seed=4), Guarded(mem, 4096, seed=5)
    beta_ok = (ctypes.c_uint32 * 4)(1, 2, 3, P - 1)
    try:
        def run(ctx=fake_ctx.ptr, e=evals.ptr, o=out.ptr, m=m, beta=beta_ok, x0=7, s=salts.ptr, lv=levels.ptr):
            return lib.toyni_fri_fold4_commit_ext_device(ctx, e, o, m, beta, x0, s, lv, None)

        nulls = {"ctx": run(ctx=None), "d_evals": run(e=None), "d_out": run(o=None), "beta": run(beta=None), "d_levels": run(lv=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        assert run(x0=0) == E_ZERO_INVERSE
        bad_beta = lambda k, v: (ctypes.c_uint32 * 4)(*[v if j == k else 5 for j in range(4)])
        ranges = {
            **{f"m {v}": run(m=v) for v in (1, 2, 4, 8, 15, 17, 24, 48, 63, (1 << 40) + 16)},       # below 16, or no power of two
            "x0 p": run(x0=P), "x0 2^32 - 1": run(x0=0xFFFFFFFF),
            **{f"beta[{k}] p": run(beta=bad_beta(k, P)) for k in range(4)}, "beta[2] 2^32 - 1": run(beta=bad_beta(2, 0xFFFFFFFF)),
            "d_evals + 4": run(e=evals.ptr + 4), "d_evals + 8": run(e=evals.ptr + 8), "d_out + 4": run(o=out.ptr + 4), "d_out + 12": run(o=out.ptr + 12),
            "d_levels + 8": run(lv=levels.ptr + 8), "d_salts + 4": run(s=salts.ptr + 4),
        }
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # nothing to do is no refusal, and writes nothing
        assert run(m=0) == 0 and run(m=0, s=None) == 0
        untouched(("evals", evals), ("out", out), ("salts", salts), ("levels", levels), ("ctx", fake_ctx))
    finally:
        for g in (evals, out, salts, levels, fake_ctx):
            g.free()


def test_every_refusal_of_the_phase_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    m0 = 64
    layer0, layers, salts = Guarded(mem, 16 * m0, seed=1), Guarded(mem, 16 * m0, seed=2), Guarded(mem, 16 * m0, seed=3)
    levels, fake_ctx, tr, betas = Guarded(mem, 32 * m0, word=1, seed=4), Guarded(mem, 4096, seed=5), Guarded(mem, 1024, seed=6), Guarded(mem, 64, seed=7)
    try:
        def run(ctx=fake_ctx.ptr, l0=layer0.ptr, m0=m0, x0=7, final=4, s=salts.ptr, t=tr.ptr, ls=layers.ptr, lv=levels.ptr, b=betas.ptr):
            return lib.toyni_fri4_commit_phase_transcript_ext_device(ctx, l0, m0, x0, final, s, t, ls, lv, b, None)

        nulls = {"ctx": run(ctx=None), "d_layer0": run(l0=None), "d_tr": run(t=None), "d_layers": run(ls=None), "d_levels": run(lv=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        sizes = {"m0 48": run(m0=48), "m0 0": run(m0=0), "m0 63": run(m0=63), "final 3": run(final=3), "final 0": run(final=0),
                 "final 1": run(final=1), "final 2": run(final=2), "final 2, m0 32": run(m0=32, final=2),             # final_size < 4
                 "odd ratio 32 / 4": run(m0=32), "odd ratio 64 / 8": run(final=8), "odd ratio 2^21 / 16": run(m0=1 << 21, final=16)}
        assert all(rc == E_INVALID_SIZE for rc in sizes.values()), sizes
        assert run(x0=0) == E_ZERO_INVERSE
        ranges = {"x0 p": run(x0=P), "x0 2^32 - 1": run(x0=0xFFFFFFFF), "d_layer0 + 4": run(l0=layer0.ptr + 4), "d_layers + 8": run(ls=layers.ptr + 8),
                  "d_levels + 8": run(lv=levels.ptr + 8), "d_salts + 12": run(s=salts.ptr + 12), "d_tr + 8": run(t=tr.ptr + 8),
                  "d_betas + 2": run(b=betas.ptr + 2)}
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        untouched(("layer0", layer0), ("layers", layers), ("salts", salts), ("levels", levels), ("ctx", fake_ctx), ("transcript", tr), ("betas", betas))
    finally:
        for g in (layer0, layers, salts, levels, fake_ctx, tr, betas):
            g.free()


def test_every_refusal_of_the_coset_calls_and_the_positions_leaves_the_outputs_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    m = 64
    layer, salts, levels = Guarded(mem, 16 * m, seed=1), Guarded(mem, 16 * (m // 4), seed=2), Guarded(mem, 32 * 31, word=1, seed=3)
    idx, out, pos = Guarded(mem, 4 * 8, seed=4), Guarded(mem, 8 * 512, seed=5), Guarded(mem, 4 * 64, seed=6)
    try:
        def commit(l=layer.ptr, m=m, s=salts.ptr, lv=levels.ptr):
            return lib.toyni_merkle_commit_cosets_ext_device(l, m, s, lv, None)

        def open_(lv=levels.ptr, m=m, l=layer.ptr, s=salts.ptr, ix=idx.ptr, nidx=8, o=out.ptr):
            return lib.toyni_merkle_open_cosets_ext_device(lv, m, l, s, ix, nidx, o, None)

        def positions(ix=idx.ptr, count=8, m0=m, final=4, o=pos.ptr):
            return lib.toyni_fri4_query_positions_device(ix, count, m0, final, o, None)

        assert commit(l=None) == E_NULL and commit(lv=None) == E_NULL
        assert all(open_(**{k: None}) == E_NULL for k in ("lv", "l", "ix", "o"))
        assert positions(ix=None) == E_NULL and positions(o=None) == E_NULL
        sizes = {f"{name} m {v}": f(m=v) for name, f in (("commit", commit), ("open", open_)) for v in (1, 2, 3, 6, 48, 63)}
        sizes.update({"positions odd ratio": positions(m0=32), "positions odd ratio 2": positions(final=8), "positions final 2": positions(final=2),
                      "positions final 1": positions(final=1)})
        assert all(rc == E_INVALID_SIZE for rc in sizes.values()), sizes
        ranges = {"commit layer + 4": commit(l=layer.ptr + 4), "commit salts + 8": commit(s=salts.ptr + 8), "commit levels + 4": commit(lv=levels.ptr + 4),
                  "commit m 2^34": commit(m=1 << 34), "open m 2^34": open_(m=1 << 34),
                  "open layer + 8": open_(l=layer.ptr + 8), "open levels + 8": open_(lv=levels.ptr + 8), "open salts + 4": open_(s=salts.ptr + 4),
                  "open out + 4": open_(o=out.ptr + 4), "open indices + 2": open_(ix=idx.ptr + 2), "open nidx 2^32": open_(nidx=1 << 32),
                  "positions indices + 2": positions(ix=idx.ptr + 2), "positions out + 1": positions(o=pos.ptr + 1), "positions m0 48": positions(m0=48),
                  "positions final 3": positions(final=3), "positions final 0": positions(final=0), "positions m0 2^33": positions(m0=1 << 33),
                  "positions count": positions(count=65537)}
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # nothing to do is no refusal, and writes nothing
        assert commit(m=0) == 0 and open_(m=0) == 0 and open_(nidx=0) == 0 and positions(count=0) == 0 and positions(m0=4) == 0 and positions(m0=2, final=4) == 0
        untouched(("layer", layer), ("salts", salts), ("levels", levels), ("indices", idx), ("records", out), ("positions", pos))
    finally:
        for g in (layer, salts, levels, idx, out, pos):
            g.free()
