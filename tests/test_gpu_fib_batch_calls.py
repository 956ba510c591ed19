"""The batch dimension of the first half of a Fibonacci proof (include/toyni_hip.h 3s) on the GPU, each of the ten calls on its own.
The specification is 3r's one sentence -- every batched call writes, for proof b, exactly the bytes the single call writes when given
proof b's pointers -- and two judges hold every case to it:

  (i)  `batch` single calls of the existing entry points on the same inputs, byte for byte;
  (ii) where a model is a few lines: the ChaCha20 keystream of tests/harness/ref_prover.py, Horner's rule, the Python transcript
       (tests/test_emu_transcript.Model), numpy.

Batches of 1, 3 and 5 lie a stride apart in ONE guard-banded buffer (the Arena of tests/test_gpu_fri_batch.py) with strides beyond the
extents, so the gaps between the proofs are guard bands too.  Shapes: N = 4 with log_blowup = 1 (the scalar paths of the quotient and
the DEEP layer), N = 256, N = 2^13; evaluation with 0, 1, POLY_CHUNK - 1, POLY_CHUNK + 1 and 300 x POLY_CHUNK coefficients; the mask
with n < mask_degree and n > mask_degree; row copies of 4, 32 and 36 bytes, 16-byte aligned and not.  A transcript whose status is set
lies in the middle of a batch, one is so long that four fields overflow it.  One sweep runs with a stride beyond 2^32 bytes, the
refusals that read a context are held on a real one, and one chain of all ten calls is captured into a graph and replayed twice."""
import ctypes

import numpy as np
import pytest

import rows_common as rc
import test_emu_transcript as emu
from harness import ref_prover
from test_gpu_fib_dz import SHIFT, fibonacci_tuple, horner, model_point, root_of_unity
from test_gpu_fri_batch import Arena

pytestmark = pytest.mark.gpu

P = 2013265921
E_RANGE = 10006
BATCHES = [1, 3, 5]
CHUNK = 4096                     # POLY_CHUNK


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


def sync(ta):
    assert ta._lib.lib.toyni_stream_synchronize(None, None) == 0


def words(rng, n):
    return rng.integers(0, P, n, dtype=np.uint64).astype(np.uint32)


def keys_of(rng, batch):
    return [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(batch)]


def put_keys(d, keys):
    return d.put(np.frombuffer(b"".join(keys), dtype=np.uint8), word=1)


def ckey(key):
    return (ctypes.c_uint8 * 32).from_buffer_copy(key)


# ---- salts ----
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("nbytes", [64, 64 * 300])
def test_fill_equals_the_single_call_and_the_keystream(ta, batch, nbytes):
    lib = ta._lib.lib
    keys = keys_of(np.random.default_rng(nbytes + batch), batch)
    with rc.Dev(ta) as d:
        a = Arena(d, batch, nbytes, nbytes + 48)
        ta.prover.chacha20_fill_batch_device(a.ptr, a.stride, nbytes, put_keys(d, keys).ptr, 3, batch)
        ones = []
        for b in range(batch):
            g = d.buf(nbytes, word=1)
            assert lib.toyni_chacha20_fill_device(g.ptr, nbytes, ckey(keys[b]), 3, None) == 0
            ones.append(g)
        sync(ta)
        got = a.get()
        for b in range(batch):
            assert (got[b] == ones[b].download(np.uint8)).all(), b
            assert (got[b] == ref_prover.chacha20_keystream(keys[b], (0, 3, 0), nbytes)).all(), b


# ---- mask ----
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("n,mask_degree", [(8, 140), (256, 140), (300, 1)])
def test_mask_equals_the_single_call_and_the_keystream_model(ta, batch, n, mask_degree):
    rng = np.random.default_rng(1000 * n + batch)
    keys = keys_of(rng, batch)
    total = n + mask_degree
    coeffs = [np.concatenate([words(rng, n), np.zeros(mask_degree, dtype=np.uint32)]) for _ in range(batch)]
    with rc.Dev(ta) as d:
        a = Arena(d, batch, 4 * total, 4 * (total + 3))
        for b in range(batch):
            a.put(b, coeffs[b])
        ta.prover.mask_poly_batch_device(a.ptr, total + 3, n, mask_degree, put_keys(d, keys).ptr, 1, batch)
        ones = [d.put(coeffs[b]) for b in range(batch)]
        for b in range(batch):
            ta.prover.mask_poly_device(ones[b].ptr, n, mask_degree, keys[b], 1)
        sync(ta)
        got = a.get(np.uint32)
        for b in range(batch):
            assert (got[b] == ones[b].download(np.uint32)).all(), b
            r = ref_prover.ChaChaRandomness(keys[b]).mask(mask_degree)
            want = [int(v) for v in coeffs[b]]
            for j in range(mask_degree):
                want[j] = (want[j] - r[j]) % P
            for j in range(mask_degree):
                want[n + j] = (want[n + j] + r[j]) % P
            assert got[b].tolist() == want, b


# ---- quotient and DEEP layer ----
SWEEPS = [(2, 1), (8, 5), (13, 5)]          # (log_N, log_blowup): the scalar paths, N = 256, more than one workgroup per proof


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("log_N,log_b", SWEEPS)
@pytest.mark.parametrize("gap,with_c", [(4, True), (5, True), (4, False)])      # gap 5: proofs 1, 3 lose the 16-byte alignment
def test_quotient_equals_the_single_call(ta, batch, log_N, log_b, gap, with_c):
    N = 1 << log_N
    rng = np.random.default_rng(77 * log_N + batch + gap)
    traces = [words(rng, N) for _ in range(batch)]
    ctx = ta.NttContext(N)
    try:
        with rc.Dev(ta) as d:
            a_t, a_c, a_q = Arena(d, batch, 4 * N, 4 * (N + gap)), Arena(d, batch, 4 * N, 4 * (N + gap)), Arena(d, batch, 4 * N, 4 * (N + gap))
            for b in range(batch):
                a_t.put(b, traces[b])
            ta.prover.fib_quotient_batch_device(ctx, a_t.ptr, N + gap, a_c.ptr if with_c else 0, N + gap, a_q.ptr, N + gap, log_b, SHIFT, batch)
            ones = []
            for b in range(batch):
                g_t, g_c, g_q = d.put(traces[b]), d.buf(4 * N), d.buf(4 * N)
                ta.prover.fib_quotient_device(ctx, g_t.ptr, g_c.ptr, g_q.ptr, log_b, SHIFT)
                ones.append((g_c, g_q))
            ctx.synchronize()
            c, q = a_c.get(np.uint32), a_q.get(np.uint32)
            for b in range(batch):
                assert (q[b] == ones[b][1].download(np.uint32)).all() and (q[b] < P).all(), b
                assert (c[b] == ones[b][0].download(np.uint32)).all() if with_c else (c[b] == 0xA5A5A5A5).all(), b
            # a stride one word short, with a context that is real
            lib = ta._lib.lib
            for ts, cs, qs in ((N - 1, N, N), (N, N - 1, N), (N, N, N - 1)):
                assert lib.toyni_fib_quotient_batch_device(ctx.handle, a_t.ptr, ts, a_c.ptr, cs, a_q.ptr, qs, log_b, SHIFT, 1, None) == E_RANGE
            assert lib.toyni_fib_quotient_batch_device(ctx.handle, a_t.ptr, N, None, 0, a_q.ptr, N, log_b, SHIFT, 0, None) == E_RANGE
    finally:
        ctx.destroy()


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("log_N,log_b", SWEEPS)
@pytest.mark.parametrize("with_check", [True, False])
def test_deep_layer_equals_the_single_call_and_its_check_word(ta, batch, log_N, log_b, with_check):
    N, n = 1 << log_N, 1 << (log_N - log_b)
    rng = np.random.default_rng(31 * log_N + batch)
    traces, quots = [words(rng, N) for _ in range(batch)], [words(rng, N) for _ in range(batch)]
    zs = [int(rng.integers(2, P)) for _ in range(batch)]
    oods = [fibonacci_tuple(rng, n, z) for z in zs]
    holds = [1] * batch
    if batch > 1:                                     # the middle proof's claim is off by one: its check word alone is 0
        oods[batch // 2][3] = (oods[batch // 2][3] + 1) % P
        holds[batch // 2] = 0
    ctx = ta.NttContext(N)
    try:
        with rc.Dev(ta) as d:
            a_t, a_q, a_o = Arena(d, batch, 4 * N, 4 * (N + 1)), Arena(d, batch, 4 * N, 4 * (N + 2)), Arena(d, batch, 4 * N, 4 * (N + 3))
            a_z, a_ood, a_chk = Arena(d, batch, 4, 12), Arena(d, batch, 16, 20), Arena(d, batch, 4, 8)
            for b in range(batch):
                a_t.put(b, traces[b]), a_q.put(b, quots[b])
                a_z.put(b, np.array([zs[b] + (P if b & 1 else 0)], dtype=np.uint32))          # odd proofs: a word that needs the reduction
                a_ood.put(b, np.array(oods[b], dtype=np.uint32))
            args = (ctx, a_t.ptr, N + 1, a_q.ptr, N + 2, a_o.ptr, N + 3, log_b, SHIFT, a_z.ptr, 3, a_ood.ptr, 5, n)
            ta.prover.fib_deep_dz_batch_device(*args, a_chk.ptr if with_check else 0, 2, batch)
            ones = []
            for b in range(batch):
                g_t, g_q, g_o = d.put(traces[b]), d.put(quots[b]), d.buf(4 * N)
                ta.prover.fib_deep_device(ctx, g_t.ptr, g_q.ptr, g_o.ptr, log_b, SHIFT, zs[b], oods[b])
                ones.append(g_o)
            ctx.synchronize()
            out, chk = a_o.get(np.uint32), a_chk.get(np.uint32)
            for b in range(batch):
                assert (out[b] == ones[b].download(np.uint32)).all(), b
                assert chk[b].tolist() == [holds[b] if with_check else 0xA5A5A5A5], b
            lib = ta._lib.lib
            ok = dict(ts=N, qs=N, os=N, zs=1, ods=4, cs=1)
            for short in ok:
                st = dict(ok, **{short: ok[short] - 1})
                assert lib.toyni_fib_deep_dz_batch_device(ctx.handle, a_t.ptr, st["ts"], a_q.ptr, st["qs"], a_o.ptr, st["os"], log_b, SHIFT, a_z.ptr, st["zs"],
                                                          a_ood.ptr, st["ods"], n, a_chk.ptr, st["cs"], 1, None) == E_RANGE, short
    finally:
        ctx.destroy()


# ---- the out-of-domain values ----
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("ncoeffs,npoints", [(0, 3), (1, 1), (CHUNK - 1, 3), (CHUNK + 1, 3), (300 * CHUNK, 2)])
def test_evaluation_equals_the_single_call_and_horner(ta, batch, ncoeffs, npoints):
    rng = np.random.default_rng(ncoeffs + 10 * batch)
    g = root_of_unity(6)
    mults = [1, g, g * g % P][:npoints]
    coeffs = [words(rng, ncoeffs) for _ in range(batch)]
    zs = [int(rng.integers(2, P)) for _ in range(batch)]
    ctx = ta.NttContext(1 << 10)
    try:
        with rc.Dev(ta) as d:
            a_c = Arena(d, batch, 4 * max(ncoeffs, 1), 4 * (ncoeffs + 3))
            a_z, a_out = Arena(d, batch, 4, 8), Arena(d, batch, 4 * npoints, 4 * (npoints + 1))
            for b in range(batch):
                if ncoeffs:
                    a_c.put(b, coeffs[b])
                a_z.put(b, np.array([zs[b] + (P if b & 1 else 0)], dtype=np.uint32))
            ta.prover.poly_eval_dz_batch_device(ctx, a_c.ptr if ncoeffs else 0, ncoeffs + 3, ncoeffs, a_z.ptr, 2, mults, batch, a_out.ptr, npoints + 1)
            ones = []
            for b in range(batch):
                g_c, g_z, g_o = d.put(coeffs[b]) if ncoeffs else None, d.put(np.array([zs[b]], dtype=np.uint32)), d.buf(4 * npoints)
                ta.prover.poly_eval_dz_device(ctx, g_c.ptr if ncoeffs else 0, ncoeffs, g_z.ptr, mults, g_o.ptr)
                ones.append(g_o)
            ctx.synchronize()
            out = a_out.get(np.uint32)
            for b in range(batch):
                assert (out[b] == ones[b].download(np.uint32)).all(), b
                if ncoeffs <= CHUNK + 1:
                    assert out[b].tolist() == [horner(coeffs[b], m * zs[b] % P) for m in mults], b
            lib = ta._lib.lib
            m = np.array(mults, dtype=np.uint32)
            for cs, zst, os_ in ((ncoeffs - 1, 1, npoints), (ncoeffs, 0, npoints), (ncoeffs, 1, npoints - 1)):
                if cs < 0:
                    continue
                assert lib.toyni_poly_eval_dz_batch_device(ctx.handle, a_c.ptr, cs, ncoeffs, a_z.ptr, zst, m.ctypes.data, npoints, 1, a_out.ptr, os_,
                                                           None) == E_RANGE
    finally:
        ctx.destroy()


# ---- the transcripts ----
def test_point_squeeze_and_field_absorb_per_transcript(ta):
    """Five transcripts: two short states (one absorbs a word that needs the reduction), one whose status is set (in the middle), one
    so long that four fields overflow it, one more plain state.  Each against its single calls and against the model."""
    pv = ta.prover
    states = [b"toyni-stark-v1" + (0).to_bytes(8, "little"), b"toyni-stark-v1" + (92).to_bytes(8, "little"), emu.pattern(60, 9),
              emu.pattern(emu.CAPACITY - 31, 4), emu.pattern(96, 2)]
    status0 = [0, 0, E_RANGE, 0, 0]
    batch = len(states)
    rng = np.random.default_rng(5)
    fields = [words(rng, 4) for _ in range(batch)]
    fields[1] = fields[1] + np.uint32(0)
    fields[1][0] = np.uint32(P + 3)                                 # a word that absorb_field reduces
    with rc.Dev(ta) as d:
        a_z, a_f = Arena(d, batch, 4, 12), Arena(d, batch, 16, 24)
        for b in range(batch):
            a_f.put(b, fields[b])
        tr = pv.DeviceTranscriptBatch.from_states(states)
        host = np.zeros(1024, dtype=np.uint8)
        host[:8] = np.array([60, E_RANGE], dtype=np.uint32).view(np.uint8)
        host[16:76] = np.frombuffer(states[2], dtype=np.uint8)
        ta._lib.check(ta._lib.lib.toyni_memcpy_h2d(tr.ptr + 2048, host.ctypes.data, 1024), "upload")
        tr.absorb_fields(a_f.ptr, 6, 4)
        tr.squeeze_point(27, SHIFT, a_z.ptr, 3)
        ones = []
        for b in range(batch):
            if status0[b]:
                ones.append(None)
                continue
            t1 = pv.DeviceTranscript.from_bytes(states[b])
            g_f, g_z = d.put(fields[b]), d.buf(4)
            t1.absorb_fields(g_f.ptr, 4)
            t1.squeeze_point(g_z.ptr, 27, SHIFT)
            ones.append((t1, g_z))
        sync(ta)
        after, z = tr.download(), a_z.get(np.uint32)
        tr.free()
        for b in range(batch):
            m = emu.Model(states[b], status0[b])
            m.absorb(b"".join((int(v) % P).to_bytes(8, "little") for v in fields[b]))
            want_z = model_point(m, 27, SHIFT)[0] if not m.status else 0
            assert z[b].tolist() == [want_z] and after[b] == (m.state, m.status), b
            if ones[b]:
                assert ones[b][1].download(np.uint32).tolist() == [want_z] and ones[b][0].download() == after[b], b
                ones[b][0].free()
        assert [s for _, s in after] == [0, 0, E_RANGE, E_RANGE, 0] and after[3][0] == states[3]


# ---- rows, roots, copies ----
@pytest.mark.parametrize("batch", BATCHES)
def test_query_rows_equal_the_single_call_and_numpy(ta, batch):
    count, n, offsets = 44, 256, [0, 32, 64]
    rng = np.random.default_rng(batch)
    idx = [rng.integers(0, n, count, dtype=np.uint64).astype(np.uint32) for _ in range(batch)]
    with rc.Dev(ta) as d:
        a_i, a_o = Arena(d, batch, 4 * count, 4 * (count + 1)), Arena(d, batch, 4 * 3 * count, 4 * (3 * count + 2))
        for b in range(batch):
            a_i.put(b, idx[b])
        ta.prover.query_rows_batch_device(a_i.ptr, count + 1, count, n, offsets, batch, a_o.ptr, 3 * count + 2)
        ones = []
        for b in range(batch):
            g_i, g_o = d.put(idx[b]), d.buf(4 * 3 * count)
            ta.prover.query_rows_device(g_i.ptr, count, n, offsets, g_o.ptr)
            ones.append(g_o)
        sync(ta)
        out = a_o.get(np.uint32)
        for b in range(batch):
            assert (out[b] == ones[b].download(np.uint32)).all(), b
            assert (out[b].reshape(count, 3) == (idx[b][:, None].astype(np.int64) + np.array(offsets)) % n).all(), b


@pytest.mark.parametrize("batch", BATCHES)
def test_phase_roots_equal_the_single_call_and_the_last_digests(ta, batch):
    lib = ta._lib.lib
    m_first, rounds = 64, 5
    ndigs = [lib.toyni_merkle_total_digests(m_first >> k) for k in range(rounds)]
    ext = 32 * sum(ndigs)
    rng = np.random.default_rng(40 + batch)
    levels = [rng.integers(0, 256, ext, dtype=np.uint8) for _ in range(batch)]
    with rc.Dev(ta) as d:
        a_l, a_r = Arena(d, batch, ext, ext + 48), Arena(d, batch, 32 * rounds, 32 * rounds + 4)
        for b in range(batch):
            a_l.put(b, levels[b])
        ta.prover.fri_phase_roots_batch_device(a_l.ptr, a_l.stride, m_first, rounds, batch, a_r.ptr, a_r.stride)
        ones = []
        for b in range(batch):
            g_l, g_r = d.put(levels[b], word=1), d.buf(32 * rounds, word=1)
            ta.prover.fri_phase_roots_device(g_l.ptr, m_first, rounds, g_r.ptr)
            ones.append(g_r)
        sync(ta)
        got = a_r.get()
        for b in range(batch):
            assert (got[b] == ones[b].download(np.uint8)).all(), b
            assert (got[b].reshape(-1, 32) == levels[b].reshape(-1, 32)[np.cumsum(ndigs) - 1]).all(), b


@pytest.mark.parametrize("rows", [1, 3, 5])
@pytest.mark.parametrize("row_bytes", [4, 32, 36, 4 * 1100])
@pytest.mark.parametrize("aligned", [True, False])
def test_row_copies_are_the_rows(ta, rows, row_bytes, aligned):
    rng = np.random.default_rng(rows * row_bytes)
    src = [rng.integers(0, 256, row_bytes, dtype=np.uint8) for _ in range(rows)]
    s_stride, d_stride = (row_bytes + 15 & ~15) + (16 if aligned else 4), (row_bytes + 15 & ~15) + (32 if aligned else 12)
    with rc.Dev(ta) as d:
        a_s, a_d = Arena(d, rows, row_bytes, s_stride), Arena(d, rows, row_bytes, d_stride)
        for r in range(rows):
            a_s.put(r, src[r])
        ta.prover.copy_rows_device(a_d.ptr, d_stride, a_s.ptr, s_stride, row_bytes, rows)
        sync(ta)
        got = a_d.get()
        assert all((got[r] == src[r]).all() for r in range(rows))
        assert all((x == y).all() for x, y in zip(a_s.get(), src))                       # the source is read only


# ---- offsets beyond 2^32 ----
def test_a_sweep_with_a_stride_beyond_four_gibibytes(ta):
    """Two proofs whose salts lie 2^32 + 64 bytes apart in one allocation, guard bands around the two regions only."""
    import torch
    dev = torch.device("cuda", 0)
    lib = ta._lib.lib
    nbytes, G, stride = 64 * 5, 1 << 16, (1 << 32) + 64
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > stride + (1 << 28), "the case needs 4 GiB of free device memory"
    keys = keys_of(np.random.default_rng(8), 2)
    big = torch.empty(G + stride + nbytes + G, dtype=torch.uint8, device=dev)
    try:
        for b in range(2):
            big[b * stride:b * stride + 2 * G + nbytes].fill_(0xA5)
        tk = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev)
        torch.cuda.synchronize()
        ta.prover.chacha20_fill_batch_device(big.data_ptr() + G, stride, nbytes, tk.data_ptr(), 0, 2)
        sync(ta)
        for b in range(2):
            region = big[b * stride:b * stride + 2 * G + nbytes].cpu().numpy()
            assert (region[:G] == 0xA5).all() and (region[G + nbytes:] == 0xA5).all(), b
            assert (region[G:G + nbytes] == ref_prover.chacha20_keystream(keys[b], (0, 0, 0), nbytes)).all(), b
    finally:
        del big
        torch.cuda.empty_cache()


# ---- captured replay ----
def test_one_chain_of_all_ten_calls_replays_from_a_captured_graph(ta):
    import torch
    pv = ta.prover
    dev = torch.device("cuda", 0)
    B, n, log_b, md = 3, 64, 1, 5
    N, log_N = n << log_b, 7
    gm = root_of_unity(6)
    mults = [1, gm, gm * gm % P]
    st_c, st_t, st_tail, st_s = n + md + 3, N + 4, 12, 128 + 16
    ctx = ta.NttContext(N)
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.uint64).astype(np.uint32)).view(np.int32)).to(dev)
    try:
        keys_t = torch.zeros(32 * B, dtype=torch.uint8, device=dev)
        coef = torch.zeros(B * st_c, dtype=torch.int32, device=dev)
        trace, quot, cev, deep = (torch.zeros(B * st_t, dtype=torch.int32, device=dev) for _ in range(4))
        tail = torch.zeros(B * st_tail, dtype=torch.int32, device=dev)        # per proof: z | 4 values | check | 6 spare words
        salts = torch.zeros(B * st_s, dtype=torch.uint8, device=dev)
        levels = torch.zeros(B, (2 * 8 - 1) + (2 * 4 - 1), 8, dtype=torch.int32, device=dev)
        roots, rows, gathered = torch.zeros(B * 16, dtype=torch.int32, device=dev), torch.zeros(B * 12, dtype=torch.int32, device=dev), torch.zeros(B * 8, dtype=torch.int32, device=dev)
        tr = pv.DeviceTranscriptBatch.from_states([b"warm"] * B)
        s = torch.cuda.Stream(device=dev)
        z, ood, chk = tail.data_ptr(), tail.data_ptr() + 4, tail.data_ptr() + 20

        def chain():
            t = s.cuda_stream
            pv.chacha20_fill_batch_device(salts.data_ptr(), st_s, 128, keys_t.data_ptr(), 0, B, t)
            pv.mask_poly_batch_device(coef.data_ptr(), st_c, n, md, keys_t.data_ptr(), 1, B, t)
            pv.fib_quotient_batch_device(ctx, trace.data_ptr(), st_t, cev.data_ptr(), st_t, quot.data_ptr(), st_t, log_b, SHIFT, B, t)
            tr.squeeze_point(log_N, SHIFT, z, st_tail, t)
            pv.poly_eval_dz_batch_device(ctx, coef.data_ptr(), st_c, n + md, z, st_tail, mults, B, ood, st_tail, t)
            pv.poly_eval_dz_batch_device(ctx, quot.data_ptr(), st_t, N, z, st_tail, mults[:1], B, ood + 12, st_tail, t)
            tr.absorb_fields(ood, st_tail, 4, t)
            pv.fib_deep_dz_batch_device(ctx, trace.data_ptr(), st_t, quot.data_ptr(), st_t, deep.data_ptr(), st_t, log_b, SHIFT, z, st_tail, ood, st_tail, n,
                                        chk, st_tail, B, t)
            pv.query_rows_batch_device(ood, st_tail, 4, N, [0, 2, 4], B, rows.data_ptr(), 12, t)
            pv.fri_phase_roots_batch_device(levels.data_ptr(), levels[0].numel() * 4, 8, 2, B, roots.data_ptr(), 64, t)
            pv.copy_rows_device(gathered.data_ptr(), 32, levels.data_ptr() + 14 * 32, levels[0].numel() * 4, 32, B, t)

        def load(seed, states):
            rng = np.random.default_rng(seed)
            keys = keys_of(rng, B)
            keys_t.copy_(torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev))
            cs = [words(rng, n) for _ in range(B)]
            ts = [words(rng, N) for _ in range(B)]
            lv = rng.integers(0, 1 << 32, levels.numel(), dtype=np.uint64)
            coef.zero_()
            for b in range(B):
                coef[b * st_c:b * st_c + n] = as_dev(cs[b])
                trace[b * st_t:b * st_t + N] = as_dev(ts[b])
            levels.copy_(as_dev(lv).reshape(levels.shape))
            tr.load(states, s.cuda_stream)
            torch.cuda.synchronize()
            return keys, cs, ts, lv.astype(np.uint32).reshape(B, -1, 8)

        load(1, [b"warm"] * B)
        chain()                                          # eager first: code objects loaded, the context's buffer holds B records
        ctx.synchronize(s.cuda_stream)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            chain()
        for seed, states in ((10, [b"first", b"second state", emu.pattern(70, 1)]), (20, [emu.pattern(33, b) for b in range(B)])):
            keys, cs, ts, lv = load(seed, states)
            for t in (tail, deep, quot, cev, roots, rows, gathered):
                t.fill_(-1)
            salts.fill_(0xA5)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            after = tr.download()
            for b in range(B):
                # the single calls on proof b's words
                t1 = pv.DeviceTranscript.from_bytes(states[b])
                c1 = torch.zeros(n + md, dtype=torch.int32, device=dev)
                c1[:n] = as_dev(cs[b])
                tr1, q1, ce1, d1 = as_dev(ts[b]), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
                tl1, r1, rw1 = torch.empty(6, dtype=torch.int32, device=dev), torch.empty(16, dtype=torch.int32, device=dev), torch.empty(12, dtype=torch.int32, device=dev)
                lv1, s1 = as_dev(lv[b].reshape(-1)), torch.empty(128, dtype=torch.uint8, device=dev)
                assert ta._lib.lib.toyni_chacha20_fill_device(s1.data_ptr(), 128, ckey(keys[b]), 0, None) == 0
                pv.mask_poly_device(c1.data_ptr(), n, md, keys[b], 1)
                pv.fib_quotient_device(ctx, tr1.data_ptr(), ce1.data_ptr(), q1.data_ptr(), log_b, SHIFT)
                t1.squeeze_point(tl1.data_ptr(), log_N, SHIFT)
                pv.poly_eval_dz_device(ctx, c1.data_ptr(), n + md, tl1.data_ptr(), mults, tl1.data_ptr() + 4)
                pv.poly_eval_dz_device(ctx, q1.data_ptr(), N, tl1.data_ptr(), mults[:1], tl1.data_ptr() + 16)
                t1.absorb_fields(tl1.data_ptr() + 4, 4)
                pv.fib_deep_dz_device(ctx, tr1.data_ptr(), q1.data_ptr(), d1.data_ptr(), log_b, SHIFT, tl1.data_ptr(), tl1.data_ptr() + 4, n, tl1.data_ptr() + 20)
                pv.query_rows_device(tl1.data_ptr() + 4, 4, N, [0, 2, 4], rw1.data_ptr())
                pv.fri_phase_roots_device(lv1.data_ptr(), 8, 2, r1.data_ptr())
                torch.cuda.synchronize()
                assert torch.equal(salts[b * st_s:][:128], s1) and (salts[b * st_s + 128:(b + 1) * st_s] == 0xA5).all(), (seed, b)
                assert torch.equal(coef[b * st_c:][:n + md], c1) and torch.equal(quot[b * st_t:][:N], q1) and torch.equal(cev[b * st_t:][:N], ce1), (seed, b)
                assert torch.equal(tail[b * st_tail:][:6], tl1) and (tail[b * st_tail + 6:(b + 1) * st_tail] == -1).all(), (seed, b)
                assert torch.equal(deep[b * st_t:][:N], d1) and (deep[b * st_t + N:(b + 1) * st_t] == -1).all(), (seed, b)
                assert torch.equal(rows[b * 12:][:12], rw1) and torch.equal(roots[b * 16:][:16], r1), (seed, b)
                assert torch.equal(gathered[b * 8:][:8], lv1[14 * 8:15 * 8]), (seed, b)
                assert after[b] == t1.download() and after[b][1] == 0, (seed, b)
                t1.free()
                # and the model: z and the state after the four fields
                m = emu.Model(states[b])
                zb = model_point(m, log_N, SHIFT)[0]
                got = tl1.cpu().numpy().view(np.uint32).tolist()
                assert got[0] == zb
                m.absorb(b"".join(int(v).to_bytes(8, "little") for v in got[1:5]))
                assert after[b][0] == m.state
        del g
        tr.free()
    finally:
        ctx.destroy()
