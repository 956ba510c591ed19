"""toyni_transcript_grind_device on the GPU (include/toyni_hip.h 3n): the nonce, the transcript after it and what is squeezed from that
transcript, against tests/pow_model.py -- hashlib alone; every expected nonce comes from that model, capped at 2^20 candidates for
bits <= 16 and 2^22 for 20 bits, and a case the model cannot answer inside its cap is an error of the test.

* every state of the checked table (lengths 0, 14, 32, 47 | 48: the one-block | two-block edge, 55, 56, 63, 64, 96, 119, 120, 1000; the
  lengths 0, 14, 55, 63, 119 put the nonce across three message words) at bits 0, 1, 8, 12, 16;
* a start below 2^32 whose answers lie beyond it; a start just past a hit; the same call twice and on a second stream; two 20-bit cases;
* the refusals the host cannot see: a window without a hit (32 bits in 2^10 tries, 24 bits in 2^12), a state that cannot take 8 bytes,
  a status that is already set -- status, *d_nonce = 0, all 1008 bytes and the length unchanged, zeros from every later squeeze;
* guard bands around the nonce word and the transcript; a captured graph replayed twice from re-uploaded states;
* end to end: tests/harness/fri4_pow_prover.py at N = 2^8, final_size 16, 8 bits -- one synchronisation, status 0 -- accepted by
  tests/harness/fri4_pow_verifier.py and rejected under the deviations of tests/test_fri4_pow_verifier_model.py.

No case asks the device for more than 2^22 candidates: the window bounds every thread's trip count."""
from functools import lru_cache

import numpy as np
import pytest

import pow_model as pm
from guarded import Guarded

pytestmark = pytest.mark.gpu

E_RANGE = pm.E_RANGE
TABLE_BITS = (0, 1, 8, 12, 16)


@pytest.fixture(scope="module")
def env():
    import __graft_entry__ as entry
    entry.build_hip()
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import toyni_amd
    return toyni_amd, torch, torch.device("cuda", 0)


@lru_cache(maxsize=None)
def expected(state, bits, start=0):
    """the model's nonce (computed once per case of the session)"""
    return pm.must_grind(state, bits, start)


class Bench:
    """one device transcript, one nonce word and two squeeze outputs, reused by the cases of a test"""

    def __init__(self, ta, torch, dev):
        self.ta, self.torch = ta, torch
        self.tr = ta.prover.DeviceTranscript()
        self.nonce = torch.full((1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
        self.chal = torch.full((4,), -1, dtype=torch.int32, device=dev)
        self.idx = torch.full((8,), -1, dtype=torch.int32, device=dev)

    def upload(self, state, status=0, length=None):
        """the transcript = `state` with stale A5 bytes behind it; a status and a length word of the caller's choice"""
        host = np.full(1024, 0xA5, dtype=np.uint8)
        host[:16] = 0
        host[:8].view(np.uint32)[:] = (len(state) if length is None else length, status)
        host[16:16 + len(state)] = np.frombuffer(bytes(state), dtype=np.uint8)
        assert self.ta._lib.lib.toyni_memcpy_h2d(self.tr.ptr, host.ctypes.data, 1024) == 0
        return host

    def raw(self):
        host = np.zeros(1024, dtype=np.uint8)
        assert self.ta._lib.lib.toyni_memcpy_d2h(host.ctypes.data, self.tr.ptr, 1024) == 0
        return host

    def grind_and_continue(self, bits, start=0, log_tries=20, stream=0):
        """grind; download; squeeze(4), squeeze_indices(8, 256) -> (nonce, state after the grind, status, challenges, indices)"""
        self.nonce.fill_(0x5A5A5A5A5A5A5A5A)
        self.torch.cuda.synchronize()
        self.tr.grind(self.nonce.data_ptr(), bits, start, log_tries, stream)
        self.torch.cuda.synchronize()
        after = self.tr.download()
        self.tr.squeeze(self.chal.data_ptr(), 4, stream)
        self.tr.squeeze_indices(self.idx.data_ptr(), 8, 256, stream)
        self.torch.cuda.synchronize()
        nonce = int(self.nonce.cpu().numpy().view(np.uint64)[0])
        return nonce, after[0], after[1], self.chal.cpu().numpy().view(np.uint32).tolist(), self.idx.cpu().numpy().view(np.uint32).tolist()

    def free(self):
        self.tr.free()


def check_against_model(b, state, bits, start=0, log_tries=20):
    m = pm.Transcript(state)
    want = expected(state, bits, start)
    assert want < start + (1 << log_tries)
    assert m.grind(bits, start, want - start + 1) == want
    b.upload(state)
    nonce, after, status, chal, idx = b.grind_and_continue(bits, start, log_tries)
    assert nonce == want, (len(state), bits, start, nonce, want)
    assert status == 0 and after == state + pm.le64(want) == m.state
    assert chal == m.squeeze(4) and idx == m.squeeze_indices(8, 256)
    return nonce


# The one-block and the two-block candidate loop live in ONE kernel symbol (the length that chooses between them is device memory), so
# the kernel-coverage guard cannot tell whether both ran: the lengths 47 (the last one-block tail) and 48 (the first two-block tail) of
# this table are what shows it.  They stay in the table.
assert {47, 48} <= {len(s) for _, s in pm.table_states()}


@pytest.mark.parametrize("name,state", pm.table_states(), ids=[n for n, _ in pm.table_states()])
def test_the_table_nonce_transcript_and_continuation_equal_the_model(env, name, state):
    b = Bench(*env)
    try:
        for bits in TABLE_BITS:
            nonce = check_against_model(b, state, bits)
            if bits == 0:
                assert nonce == 0                                   # bits = 0 accepts the first candidate, and still absorbs it
    finally:
        b.free()


def test_a_start_below_2_32_whose_answers_lie_beyond_it(env):
    b = Bench(*env)
    try:
        start, s = (1 << 32) - 100, pm.pattern(64, 3)
        assert check_against_model(b, s, 8, start) == start + 232
        assert check_against_model(b, s, 12, start) == start + 3345
        assert check_against_model(b, s, 0, start) == start
        top = (1 << 64) - (1 << 12)                                 # the window that ends at 2^64 exactly
        assert check_against_model(b, s, 8, top, 12) >= top
    finally:
        b.free()


def test_a_start_at_and_just_past_a_hit(env):
    b = Bench(*env)
    try:
        for s in (pm.START_STATE, pm.pattern(63, 63)):
            first = expected(s, 12)
            assert check_against_model(b, s, 12, first) == first
            second = check_against_model(b, s, 12, first + 1)
            assert second > first and second == pm.must_grind(s, 12, first + 1)
    finally:
        b.free()


def test_the_same_call_twice_and_on_a_second_stream_gives_the_same_answer(env):
    ta, torch, dev = env
    b = Bench(*env)
    try:
        s2 = torch.cuda.Stream(device=dev)
        for state, bits in ((pm.pattern(64, 64), 16), (pm.pattern(55, 55), 12)):
            runs = []
            for stream in (0, 0, s2.cuda_stream):
                b.upload(state)
                runs.append(b.grind_and_continue(bits, 0, 20, stream))
            assert runs[0] == runs[1] == runs[2] and runs[0][0] == expected(state, bits)
    finally:
        b.free()


@pytest.mark.parametrize("state", [pm.START_STATE, pm.pattern(64, 1)], ids=["toyni-stark-v1", "pattern(64,1)"])
def test_twenty_bits(env, state):
    b = Bench(*env)
    try:
        nonce = check_against_model(b, state, 20, 0, 22)
        assert nonce == {pm.START_STATE: 1371585, pm.pattern(64, 1): 2008232}[state]
    finally:
        b.free()


def expect_refused(b, host_before, status_after, result):
    """after a refused grind: the status, *d_nonce = 0, the length word and all 1008 bytes as uploaded, zeros from later squeezes"""
    nonce, _, status, chal, idx = result
    raw = b.raw()
    assert status == status_after and nonce == 0
    assert (raw[16:] == host_before[16:]).all() and (raw[:4] == host_before[:4]).all() and (raw[8:16] == 0).all()
    assert raw[4:8].view(np.uint32)[0] == status_after
    assert chal == [0] * 4 and idx == [0] * 8


def test_a_window_without_a_hit_sets_the_status_and_leaves_the_state(env):
    b = Bench(*env)
    try:
        s = pm.pattern(64, 9)
        for bits, log_tries in ((32, 10), (24, 12)):
            assert pm.grind(s, bits, 0, 1 << log_tries) is None
            host = b.upload(s)
            expect_refused(b, host, E_RANGE, b.grind_and_continue(bits, 0, log_tries))
    finally:
        b.free()


def test_a_state_that_cannot_take_the_nonce_and_a_status_already_set(env):
    b = Bench(*env)
    try:
        for n in (1001, 1008):
            host = b.upload(pm.pattern(n, 5))
            expect_refused(b, host, E_RANGE, b.grind_and_continue(1, 0, 10))
        host = b.upload(pm.pattern(2000, 5)[:1008], length=2000)    # a length word no state can have
        expect_refused(b, host, E_RANGE, b.grind_and_continue(0, 0, 10))
        host = b.upload(pm.pattern(64, 9), status=7)
        expect_refused(b, host, 7, b.grind_and_continue(0, 0, 10))
        # 1000 bytes is the longest state that takes a nonce: 15 full blocks in the midstate, the 1008 bytes full afterwards
        check_against_model(b, pm.pattern(1000, 1000), 8)
    finally:
        b.free()


@pytest.mark.parametrize("offset", [0, 8])
def test_nothing_outside_the_nonce_word_and_the_transcript_is_written(env, offset):
    ta, torch, dev = env
    lib = ta._lib.lib
    tr, nonce = Guarded(ta, 1024, seed=1), Guarded(ta, 8, offset=offset, seed=2)
    try:
        for pattern in ("sentinel", "random"):
            for state, bits, lt in ((pm.pattern(63, 63), 12, 20), (pm.pattern(1000, 1000), 8, 20), (pm.pattern(64, 9), 24, 12), (pm.pattern(1008, 5), 1, 10)):
                tr.refill(pattern), nonce.refill(pattern)
                host = np.full(1024, 0xA5, dtype=np.uint8)
                host[:16] = 0
                host[:4].view(np.uint32)[0] = len(state)
                host[16:16 + len(state)] = np.frombuffer(state, dtype=np.uint8)
                tr.upload(host)
                assert lib.toyni_transcript_grind_device(tr.ptr, bits, 0, lt, nonce.ptr, None) == 0
                torch.cuda.synchronize()
                m = pm.Transcript(state)
                want = m.grind(bits, 0, 1 << lt)
                got = tr.download(np.uint8)
                assert int(nonce.download(np.uint64)[0]) == want
                assert got[:8].view(np.uint32).tolist() == [len(m.state), m.status] and got[16:16 + len(m.state)].tobytes() == m.state
                assert (got[16 + len(m.state):] == 0xA5).all() and (got[8:16] == 0).all()
                tr.check("transcript"), nonce.check("nonce")
    finally:
        tr.free()
        nonce.free()


def test_a_captured_graph_replays_the_chain_from_re_uploaded_states(env):
    ta, torch, dev = env
    b = Bench(*env)
    try:
        s = torch.cuda.Stream(device=dev)

        def call():
            b.tr.grind(b.nonce.data_ptr(), 12, 0, 20, s.cuda_stream)
            b.tr.squeeze_indices(b.idx.data_ptr(), 8, 256, s.cuda_stream)

        b.upload(b"warm")
        torch.cuda.synchronize()
        call()                                                      # eager first: every launch site has filed its kernel
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        for state in (pm.pattern(47, 47), pm.pattern(48, 48), pm.pattern(64, 9)):
            b.upload(state)
            b.nonce.fill_(-1), b.idx.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            m = pm.Transcript(state)
            want = m.grind(12)
            want_idx = m.squeeze_indices(8, 256)
            assert int(b.nonce.cpu().numpy().view(np.uint64)[0]) == want == expected(state, 12)
            assert b.idx.cpu().numpy().view(np.uint32).tolist() == want_idx and b.tr.download() == (m.state, 0)
        del g
    finally:
        b.free()


# ---- end to end: a ground low-degree proof ----
# (two four-to-one rounds from 2^8 to 16 divide the degree bound by 16: 16 coefficients, blow-up 16, leave a constant final layer)
N_EXT, LOG_BLOWUP, SHIFT, FINAL, BITS = 1 << 8, 4, 7, 16, 8


def test_a_ground_proof_end_to_end_is_accepted_and_each_deviation_rejected(env, monkeypatch):
    ta, torch, dev = env
    from harness import fri4_ext_verifier as fv, fri4_pow_prover as fp, fri4_pow_verifier as pv
    assert pv.POW_BITS == BITS
    ctx = ta.ntt.get_or_create_ctx(N_EXT)
    coeffs = np.random.default_rng(8).integers(0, pm.P, (N_EXT >> LOG_BLOWUP, 4), dtype=np.uint64)

    def prove(bits=BITS, **kw):
        return fp.prove(ctx, coeffs, LOG_BLOWUP, SHIFT, FINAL, pv.SEED, pv.NQUERIES, np.random.default_rng(81), bits, **kw)

    syncs, real_sync = [], torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (syncs.append(1), real_sync(*a, **k))[1])
    proof, extras = prove()
    monkeypatch.undo()
    assert len(syncs) == 1 and extras["status"] == 0                # one synchronisation from the coefficients to the records
    state = pv.state_before_queries(proof)
    nonce = proof["pow_nonce"]
    assert len(state) == 64 and nonce == expected(state, BITS) and proof["pow_bits"] == BITS
    assert (extras["betas"], extras["indices"]) == pv.challenges(proof)
    assert pv.verify(proof) == (True, "accepted")
    assert len(proof["roots"]) == 2 and len(proof["final_layer"]) == FINAL and len(set(proof["final_layer"])) == 1
    assert fv.verify(proof)[0] is False                             # the ungrinded verifier reads other leaves
    # nonce + 1
    assert not pm.accept(state, nonce + 1, BITS)
    ok, why = pv.verify(dict(proof, pow_nonce=nonce + 1))
    assert not ok and why.startswith("proof of work"), why
    # a nonce good for BITS - 1 only, ground and absorbed by the device, presented for BITS
    weak = next(n for n in range(1 << 20) if pm.accept(state, n, BITS - 1) and not pm.accept(state, n, BITS))
    cheap, ex = prove(BITS - 1, start=weak)
    assert ex["status"] == 0 and cheap["pow_nonce"] == weak and cheap["roots"] == proof["roots"]
    assert pv.verify(cheap, pow_bits=BITS - 1) == (True, "accepted")
    ok, why = pv.verify(dict(cheap, pow_bits=BITS))
    assert not ok and why.startswith("proof of work: the hash"), why
    # the nonce found but not absorbed before the indices
    skipped, ex = prove(absorb=False)
    assert ex["status"] == 0 and skipped["pow_nonce"] == nonce and ex["indices"] == fv.challenges(skipped)[1]
    ok, why = pv.verify(skipped)
    assert not ok and why.startswith("query 0, layer 0"), why
    # a larger accepted nonce is still accepted: minimality is the prover's determinism, not a verifier rule
    later, ex = prove(start=nonce + 1)
    assert ex["status"] == 0 and later["pow_nonce"] == expected(state, BITS, nonce + 1) > nonce
    assert pv.verify(later) == (True, "accepted")
    # bits = 0 still absorbs a nonce (0): NOT the ungrinded protocol's proof -- the indices differ from it through the 8 absorbed
    # bytes and through nothing else (replayed with hashlib)
    zero, ex = prove(0)
    assert ex["status"] == 0 and zero["pow_nonce"] == 0 and zero["roots"] == proof["roots"] and ex["betas"] == extras["betas"]
    replay = pm.Transcript(state + pm.le64(0))
    assert ex["indices"] == replay.squeeze_indices(pv.NQUERIES, N_EXT // 4) != fv.challenges(zero)[1]
    assert fv.challenges(zero)[1] == pm.Transcript(state).squeeze_indices(pv.NQUERIES, N_EXT // 4)
    assert pv.verify(zero, pow_bits=0) == (True, "accepted") and pv.verify(zero) == (False, "proof of work: bits or nonce field")
