"""The batch dimension of the tail (include/toyni_hip.h 3r): the six entry points are exported with the header's parameter counts and
bound in the Python package, and every refusal the host decides before anything is enqueued comes from an otherwise valid call with
the outputs untouched.  The pointers are host stand-in memory (tests/guarded.py HostMem), the context a block of it that a call which
passed its checks would misread -- none does.  The order of the refusals is the header's: null pointers, batch, the single call's own
in the single call's order (held here against the single call itself on the same bad arguments), the strides.  No compute."""
import ctypes
import os

import numpy as np
import pytest

from guarded import Guarded, HostMem, P

E_INVALID_SIZE, E_NULL, E_ZERO_INVERSE, E_RANGE = 10001, 10002, 10005, 10006
COUNTS = {"toyni_merkle_commit_batch_device": 9, "toyni_transcript_absorb_batch_device": 6, "toyni_fri_commit_phase_transcript_batch_device": 17,
          "toyni_fri_commit_phase_transcript_ext_batch_device": 17, "toyni_transcript_squeeze_indices_batch_device": 7,
          "toyni_fri_query_positions_batch_device": 9}


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    return toyni_amd


def test_symbols_are_exported_and_bound_with_the_headers_parameter_counts(ta):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "toyni_hip.h")).read()
    assert " * 3r. " in header and header.index(" * 3r. ") > header.index(" * 3q. ")
    for name, nargs in COUNTS.items():
        assert name in ta._lib.SIGNATURES and hasattr(ta._lib.lib, name), name
        f = getattr(ta._lib.lib, name)
        assert f.argtypes == ta._lib.SIGNATURES[name][1] and len(f.argtypes) == nargs and f.restype is ctypes.c_int
        decl = header.split("int " + name + "(", 1)[1].split(");", 1)[0]
        assert decl.count(",") + 1 == nargs, (name, decl)
    sig = ta._lib.SIGNATURES
    assert sig["toyni_fri_commit_phase_transcript_batch_device"][1] == sig["toyni_fri_commit_phase_transcript_ext_batch_device"][1]
    # every stride is a size_t
    assert sig["toyni_merkle_commit_batch_device"][1] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                          ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert hasattr(ta, "merkle_commit_batch_device")
    for name in ("DeviceTranscriptBatch", "fri_commit_phase_transcript_batch_device", "fri_commit_phase_transcript_ext_batch_device",
                 "fri_query_positions_batch_device"):
        assert hasattr(ta.prover, name)
    for method in ("from_states", "absorb_device", "squeeze_indices", "download", "status"):
        assert hasattr(ta.prover.DeviceTranscriptBatch, method)


def _untouched(buffers):
    for name, g in buffers:
        g.check(name)
        assert (g.download(np.uint8) == 0xA5).all(), name


def test_every_refusal_of_the_small_calls_leaves_everything_untouched(ta):
    lib = ta._lib.lib
    mem = HostMem()
    n, B = 5, 3
    ndig = lib.toyni_merkle_total_digests(n)
    assert ndig == 5 + 3 + 2 + 1
    tr, data, out, idx = Guarded(mem, 1024 * B, seed=1), Guarded(mem, 4096, word=1, seed=2), Guarded(mem, 4 * 65536, seed=3), Guarded(mem, 4 * 1024, seed=4)
    vals, salts, levels = Guarded(mem, 4 * 64, seed=5), Guarded(mem, 16 * 64, word=1, seed=6), Guarded(mem, 32 * 64, word=1, seed=7)
    try:
        def commit(v=vals.ptr, vs=n + 3, s=salts.ptr, ss=16 * n + 16, n=n, b=B, lv=levels.ptr, ls=32 * ndig + 16):
            return lib.toyni_merkle_commit_batch_device(v, vs, s, ss, n, b, lv, ls, None)

        def absorb(t=tr.ptr, b=B, d=data.ptr, st=40, n=32):
            return lib.toyni_transcript_absorb_batch_device(t, b, d, st, n, None)

        def indices(t=tr.ptr, b=B, n=8, mx=64, o=out.ptr, st=9):
            return lib.toyni_transcript_squeeze_indices_batch_device(t, b, n, mx, o, st, None)

        def positions(i=idx.ptr, ist=9, n=8, m0=64, fin=4, b=B, o=out.ptr, ost=4 * 2 * 8 + 1):
            return lib.toyni_fri_query_positions_batch_device(i, ist, n, m0, fin, b, o, ost, None)

        nulls = {"commit values": commit(v=None), "commit levels": commit(lv=None), "absorb tr": absorb(t=None), "absorb bytes": absorb(d=None),
                 "indices tr": indices(t=None), "indices out": indices(o=None), "positions idx": positions(i=None), "positions out": positions(o=None)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        # a null pointer is named before a bad batch
        assert commit(v=None, b=0) == E_NULL and absorb(t=None, b=1 << 16) == E_NULL and indices(o=None, b=0) == E_NULL and positions(i=None, b=0) == E_NULL
        ranges = {}
        for b in (0, 65536, 1 << 40):
            ranges.update({f"commit batch {b}": commit(b=b), f"absorb batch {b}": absorb(b=b), f"indices batch {b}": indices(b=b),
                           f"positions batch {b}": positions(b=b)})
        ranges.update({
            # the single calls' own
            "commit levels + 8": commit(lv=levels.ptr + 8), "commit salts + 4": commit(s=salts.ptr + 4),
            "absorb tr + 4": absorb(t=tr.ptr + 4), "absorb 1009": absorb(n=1009, st=2000), "absorb 2^40": absorb(n=1 << 40, st=1 << 41),
            "indices tr + 12": indices(t=tr.ptr + 12), "indices out + 1": indices(o=out.ptr + 1), "indices count 0": indices(n=0),
            "indices count 257": indices(n=257, mx=1 << 20, st=300), "indices max 0": indices(mx=0), "indices count > max": indices(n=9, mx=8),
            "positions idx + 2": positions(i=idx.ptr + 2), "positions out + 3": positions(o=out.ptr + 3), "positions m0 48": positions(m0=48),
            "positions m0 0": positions(m0=0), "positions final 3": positions(fin=3), "positions final 0": positions(fin=0),
            "positions m0 2^33": positions(m0=1 << 33), "positions count 65537": positions(n=65537, ist=1 << 20, ost=1 << 30),
            # a stride one element short of the extent, and one that breaks the alignment rule
            "commit value_stride n - 1": commit(vs=n - 1), "commit salt_stride 16 n - 1": commit(ss=16 * n - 1),
            "commit salt_stride 16 n - 16": commit(ss=16 * n - 16), "commit salt_stride + 8": commit(ss=16 * n + 8),
            "commit level_stride - 1": commit(ls=32 * ndig - 1), "commit level_stride - 16": commit(ls=32 * ndig - 16),
            "commit level_stride + 8": commit(ls=32 * ndig + 8), "commit level_stride 0": commit(ls=0),
            "absorb byte_stride 31": absorb(st=31), "absorb byte_stride 0": absorb(st=0),
            "indices out_stride 7": indices(st=7), "indices out_stride 0": indices(st=0),
            "positions index_stride 7": positions(ist=7), "positions out_stride 63": positions(ost=4 * 2 * 8 - 1),
        })
        assert all(rc == E_RANGE for rc in ranges.values()), ranges
        # the strides of a null d_salts are not looked at -- but the call would then enqueue, so it is only held not to name the stride:
        # (covered on the GPU).  Exact extents are accepted up to the point where nothing is left to do:
        # batch = 65535 passes the argument check (nothing to do is no refusal and enqueues nothing; no device is needed to say so)
        assert commit(n=0, b=65535) == 0 and commit(n=0, b=65536) == E_RANGE
        assert absorb(n=0, st=0, b=65535) == 0 and absorb(d=None, n=0, st=0, b=65535) == 0 and absorb(n=0, st=0, b=65536) == E_RANGE
        assert positions(n=0, b=65535) == 0 and positions(m0=4, fin=4, ost=0, b=65535) == 0 and positions(m0=4, fin=16, ost=0, b=65535) == 0
        assert positions(n=0, b=65536) == E_RANGE
        _untouched((("tr", tr), ("data", data), ("out", out), ("idx", idx), ("values", vals), ("salts", salts), ("levels", levels)))
    finally:
        for g in (tr, data, out, idx, vals, salts, levels):
            g.free()


def _digests(lib, m0, final):
    total, m = 0, m0
    while m > final:
        m //= 2
        total += lib.toyni_merkle_total_digests(m)
    return total


@pytest.mark.parametrize("ext", [False, True])
def test_every_refusal_of_the_phases_leaves_everything_untouched(ta, ext):
    lib = ta._lib.lib
    mem = HostMem()
    m0, fin, B, W = 64, 4, 3, 4 if ext else 1
    rounds = 4
    ndig = _digests(lib, m0, fin)
    layer0, layers, salts = Guarded(mem, 16 * m0 * B + 4096, seed=1), Guarded(mem, 16 * m0 * B + 4096, seed=2), Guarded(mem, 16 * m0 * B + 4096, seed=3)
    levels, fake_ctx = Guarded(mem, (32 * ndig + 64) * B, word=1, seed=4), Guarded(mem, 4096, seed=5)
    tr, betas = Guarded(mem, 1024 * B, seed=6), Guarded(mem, 4 * 4 * 8 * B, seed=7)
    single = lib.toyni_fri_commit_phase_transcript_ext_device if ext else lib.toyni_fri_commit_phase_transcript_device
    entry = lib.toyni_fri_commit_phase_transcript_ext_batch_device if ext else lib.toyni_fri_commit_phase_transcript_batch_device
    ext0 = {"l0s": W * m0, "ss": 16 * (m0 - 2 * fin), "lss": W * (m0 - fin), "lvs": 32 * ndig, "bs": W * rounds}     # the exact extents
    try:
        def run(ctx=fake_ctx.ptr, l0=layer0.ptr, l0s=ext0["l0s"] + 4, m0=m0, x0=7, final=fin, s=salts.ptr, ss=ext0["ss"] + 16, t=tr.ptr, b=B,
                ls=layers.ptr, lss=ext0["lss"] + 4, lv=levels.ptr, lvs=ext0["lvs"] + 16, bt=betas.ptr, bs=ext0["bs"] + 1):
            return entry(ctx, l0, l0s, m0, x0, final, s, ss, t, b, ls, lss, lv, lvs, bt, bs, None)

        def one(ctx=fake_ctx.ptr, l0=layer0.ptr, m0=m0, x0=7, final=fin, s=salts.ptr, t=tr.ptr, ls=layers.ptr, lv=levels.ptr, bt=betas.ptr):
            return single(ctx, l0, m0, x0, final, s, t, ls, lv, bt, None)

        nulls = {"ctx": run(ctx=None), "d_layer0": run(l0=None), "d_tr": run(t=None), "d_layers": run(ls=None), "d_levels": run(lv=None),
                 "ctx, batch 0": run(ctx=None, b=0), "d_tr, m0 48": run(t=None, m0=48)}
        assert all(rc == E_NULL for rc in nulls.values()), nulls
        batches = {b: run(b=b) for b in (0, 65536, 1 << 33)}
        assert all(rc == E_RANGE for rc in batches.values()), batches
        assert run(b=0, m0=48) == E_RANGE and run(b=65536, x0=0) == E_RANGE              # batch before the single call's own
        # the single call's refusals with its codes, and in its order: the same bad arguments, alone and in pairs, through both calls
        bad = {"m0 48": dict(m0=48), "m0 0": dict(m0=0), "final 3": dict(final=3), "final 0": dict(final=0), "m0 63": dict(m0=63), "x0 0": dict(x0=0),
               "x0 p": dict(x0=P), "x0 2^32 - 1": dict(x0=0xFFFFFFFF), "d_levels + 8": dict(lv=levels.ptr + 8), "d_salts + 12": dict(s=salts.ptr + 12),
               "d_tr + 4": dict(t=tr.ptr + 4), "d_tr + 8": dict(t=tr.ptr + 8), "d_betas + 2": dict(bt=betas.ptr + 2),
               "d_layer0 + 4": dict(l0=layer0.ptr + 4), "d_layers + 8": dict(ls=layers.ptr + 8)}
        if not ext:                                                    # the base call reads its layers word by word
            del bad["d_layer0 + 4"], bad["d_layers + 8"]
        names = sorted(bad)
        for i, a in enumerate(names):
            want = one(**bad[a])
            assert want != 0 and run(**bad[a]) == want, a
            for c in names[i + 1:]:
                if set(bad[a]) & set(bad[c]):
                    continue
                both = dict(bad[a], **bad[c])
                assert run(**both) == one(**both), (a, c)
            assert run(**dict(bad[a], lvs=0)) == want, a                # ... and before the strides
        assert one(x0=0) == (E_ZERO_INVERSE if ext else E_RANGE) and one(m0=48) == E_INVALID_SIZE
        # a stride one element short of the extent, and one that breaks the alignment rule of its pointer
        strides = {"layer0 - 1": run(l0s=ext0["l0s"] - 1), "layers - 1": run(lss=ext0["lss"] - 1), "salts - 1": run(ss=ext0["ss"] - 1),
                   "salts - 16": run(ss=ext0["ss"] - 16), "salts + 8": run(ss=ext0["ss"] + 8), "levels - 1": run(lvs=ext0["lvs"] - 1),
                   "levels - 16": run(lvs=ext0["lvs"] - 16), "levels + 8": run(lvs=ext0["lvs"] + 8), "betas - 1": run(bs=ext0["bs"] - 1),
                   "all zero": run(l0s=0, ss=0, lss=0, lvs=0, bs=0)}
        if ext:
            strides.update({"layer0 - 4": run(l0s=ext0["l0s"] - 4), "layer0 + 2": run(l0s=ext0["l0s"] + 2), "layers + 1": run(lss=ext0["lss"] + 1)})
        assert all(rc == E_RANGE for rc in strides.values()), strides
        # nothing to fold is no refusal; there batch = 65535 passes the argument check and 65536 does not
        assert run(m0=4, final=4, b=65535) == 0 and run(m0=4, final=16, b=65535) == 0 and run(m0=4, final=4, b=65536) == E_RANGE
        assert run(m0=4, final=4, b=65535, s=None, ss=0, bt=None, bs=0) == 0     # the stride of a null pointer is not looked at
        _untouched((("layer0", layer0), ("layers", layers), ("salts", salts), ("levels", levels), ("ctx", fake_ctx), ("tr", tr), ("betas", betas)))
    finally:
        for g in (layer0, layers, salts, levels, fake_ctx, tr, betas):
            g.free()
