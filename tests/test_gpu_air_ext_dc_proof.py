"""The staged AIR proof under Ext challenges with the transcript on the device from the FIRST root onward
(tests/harness/air_ext_dc_prover.py: the sequence of include/toyni_hip.h 3p, then 3o), against the two judges of
tests/test_gpu_air_ext_dz_proof.py that never saw the device:
  1. the oracle-only prover (tests/harness/air_ext_ref_prover.py): the same proof byte for byte
  2. the verifier (tests/harness/air_ext_verifier.py): accepts it, the transcript's final status 0 -- and rejects the proof of a false
     trace, which is byte for byte the reference's proof of it.
Sizes (n, log2 B) as there: (16, 1) everything single-workgroup, the scans one tile; (256, 2); (4096, 2), where the scans take the
three-launch path (four tiles of 1024).
The harness's claims are counted, not trusted: with every way it has to read device memory wrapped for the length of one proof, NOTHING
is read and nothing synchronises before "final download" -- not between loading the transcript and the download, and not before the
load either (the dz harness reads three roots there) -- exactly one synchronisation follows, and the constraint program is created
once for all the proofs of this module on a context."""
import functools

import pytest

from harness import air_ext_ref_prover as ref
from harness import air_ext_verifier as av
from harness.fib_verifier import P

pytestmark = pytest.mark.gpu

CASES = [(16, 1, 0), (256, 2, 0), (4096, 2, 0)]          # n, log2 B, seed
FALSE_AT = (64, 2, 2)


@pytest.fixture(scope="module")
def prover():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    from harness import air_ext_dc_prover
    return air_ext_dc_prover


@functools.lru_cache(maxsize=None)
def reference(n, log_b, seed, wrong=None):
    main = ref.true_main(n, seed)
    if wrong == "b":
        main[1, n // 3] = (main[1, n // 3] + 1) % P
    main.setflags(write=False)
    return main, ref.prove(main, log_b, seed)[0]


@pytest.mark.parametrize("n,log_b,seed", CASES)
def test_device_challenge_proof_equals_the_reference_proof_and_verifies(prover, n, log_b, seed):
    main, want = reference(n, log_b, seed)
    info = {}
    got = prover.prove(main, log_b, seed, info)
    assert ref.first_proof_difference(got, want) == ""
    assert set(got) == set(ref.WIRE_FIELDS) and bytes(got["opening_records"]) == bytes(want["opening_records"])
    assert info["transcript_status"] == 0
    why = []
    assert av.verify(got, why), why


def test_the_proof_of_a_false_trace_is_the_reference_proof_of_it_and_is_rejected(prover):
    n, log_b, seed = FALSE_AT
    main, want = reference(n, log_b, seed, "b")
    info = {}
    got = prover.prove(main, log_b, seed, info)
    assert ref.first_proof_difference(got, want) == "" and bytes(got["opening_records"]) == bytes(want["opening_records"])
    assert info["transcript_status"] == 0
    why = []
    assert av.verify(got, why) is False and why == ["ood"]


def test_nothing_is_read_back_before_the_final_download_and_the_program_is_created_once(prover, monkeypatch):
    import torch
    import toyni_amd
    lib = toyni_amd._lib.lib
    events = prover.EVENTS
    n, log_b, seed = CASES[1]
    main, want = reference(n, log_b, seed)
    prover.prove(main, log_b, seed)              # (the context's program exists from here on, whatever ran before)
    created = len(prover.CREATED)
    del events[:]

    def counted(name, fn):
        def wrapper(*a, **k):
            events.append(name)
            return fn(*a, **k)
        return wrapper

    for name in ("cpu", "item", "tolist", "numpy"):
        monkeypatch.setattr(torch.Tensor, name, counted("read: Tensor." + name, getattr(torch.Tensor, name)))
    monkeypatch.setattr(torch.cuda, "synchronize", counted("sync: torch.cuda.synchronize", torch.cuda.synchronize))
    for name in ("toyni_memcpy_d2h", "toyni_memcpy_d2h_async", "toyni_stream_synchronize"):
        monkeypatch.setattr(lib, name, counted("read: " + name, getattr(lib, name)), raising=False)
    for name in ("toyni_air_program_create", "toyni_air_program_create_params"):
        monkeypatch.setattr(lib, name, counted("create: " + name, getattr(lib, name)), raising=False)
    got = prover.prove(main, log_b, seed)
    monkeypatch.undo()
    assert ref.first_proof_difference(got, want) == ""
    lo, hi = events.index("transcript loaded"), events.index("final download")
    assert lo < hi and events[lo + 1:hi] == [], events[lo + 1:hi]
    before, after = events[:lo], events[hi + 1:]
    assert before == [], before                  # the dz harness reads three roots here
    assert after[0] == "sync: torch.cuda.synchronize" and sum(e.startswith("sync") for e in after) == 1
    assert sum(e.startswith("read") for e in after) >= 8, "the three roots are among the final downloads"
    assert not any(e.startswith("create") for e in events) and len(prover.CREATED) == created, "one program per AIR, not per proof"
    del events[:]
