"""Column passes whose workgroups stay on one column tile look their twiddle seeds up once per launch (PassArgs::seeds_invariant,
seeds_launch_invariant in toyni_amd/csrc/ntt_route.hpp); the others once per tile.  Through the C ABI with the default dispatch, word
for word against the oracle on the first, the last and two middle transforms of the batch, and the forward + inverse round trip on
the whole batch:

    24 x 2^20            768 32-wide tiles, 32 per prefix: three per workgroup on 256 CUs, paired tile order -- seeds looked up once
    16 x 2^20 inverse    the n^-1 factor rides on the hoisted seed
     2 x 2^24            first pass: 1024 64-wide tiles per prefix, more than the grid -- per-tile seeds; middle pass: 4 per prefix -- once
    64 x 2^18            512-point column pass, 16 tiles per prefix
    16 x 2^20 coset      the forward coset seed of the first pass is hoisted with the twiddle seeds
     4 x 2^20 Ext        interleaved columns: 128 tiles per prefix

(which of the two forms a launch takes depends on the device's CU count; tests/test_seed_hoist_predicate.py and
tests/test_emu_seed_hoist.py pin the rule and both forms of the loop on the CPU).  Bit-exact: integer path, no tolerance."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
from test_gpu_parity import DevBuf, ta  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

DEAD = 0xDEADBEEF                      # >= p: no output word can equal it


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(max_workers=8) as ex:
        yield ex


def oracle_transform(x, n, inverse, shift):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    if shift == 1:
        return oracle.intt(x) if inverse else oracle.ntt(x)
    return oracle.domain_ifft(x, shift) if inverse else oracle.domain_fft(x, n, shift)


def _job(label, got, x, n, inverse, shift):
    want = oracle_transform(x, n, inverse, shift)
    if np.array_equal(got, want):
        return None
    bad = np.flatnonzero(got != want)
    return f"{label}: {bad.size} of {want.size} words differ from the oracle, first at index {int(bad[0])}"


def settle(futures):
    errors = [e for e in (f.result() for f in futures) if e]
    assert not errors, "\n".join(errors)


def run(ta, x32, n, count, inverse, inplace, shift=1, ext=False):
    """One device call on `count` transforms (ext: Ext vectors, [count][n][4]); out of place: output prefilled, input checked."""
    ctx = ta.ntt.get_or_create_ctx(n)
    guard = 4 * n * (4 if ext else 1)
    a = DevBuf(ta, x32.nbytes, guard=guard)
    b = a if inplace else DevBuf(ta, x32.nbytes, guard=guard)
    try:
        a.upload(x32)
        if not inplace:
            b.upload(np.full(x32.size, DEAD, dtype=np.uint32))
        if ext:
            ctx.run_device_ext_batch(a.ptr, b.ptr, count, inverse, shift=shift)
        else:
            ctx.run_device(a.ptr, b.ptr, count, inverse, shift=shift)
        ctx.synchronize()
        got = b.download(np.uint32, x32.size)
        if not inplace:
            assert np.array_equal(a.download(np.uint32, x32.size), x32), "out-of-place transform modified its input"
    finally:
        a.free()
        if b is not a:
            b.free()
    return got


def four_rows(batch):
    return sorted({0, batch // 3, (2 * batch) // 3, batch - 1})


@pytest.mark.parametrize("log_n,batch,inverse,shift", [(20, 24, False, 1), (20, 16, True, 1), (24, 2, False, 1), (18, 64, False, 1), (20, 16, False, 7)],
                         ids=["24x2^20", "16x2^20-inverse", "2x2^24", "64x2^18", "16x2^20-coset"])
def test_batches_against_the_oracle_and_round_trip(ta, pool, log_n, batch, inverse, shift):
    n = 1 << log_n
    x32 = oracle.splitmix(n * batch, 0x5EED + 64 * log_n + batch + (1 if inverse else 0)).astype(np.uint32)
    got = run(ta, x32, n, batch, inverse, inplace=False, shift=shift)
    futures = [pool.submit(_job, f"2^{log_n} x{batch} inverse={inverse} shift={shift} transform {t}", got[t * n:(t + 1) * n], x32[t * n:(t + 1) * n], n, inverse, shift)
               for t in four_rows(batch)]
    back = run(ta, got, n, batch, not inverse, inplace=True, shift=shift)      # the whole batch, the other direction
    assert np.array_equal(back, x32), "whole-batch round trip"
    settle(futures)


def test_ext_vectors_against_the_oracle_and_round_trip(ta, pool):
    log_n, vecs = 20, 4
    n = 1 << log_n
    x = oracle.splitmix(4 * n * vecs, 0xE875EED).astype(np.uint32).reshape(vecs, n, 4)
    got = run(ta, x.reshape(-1), n, vecs, False, inplace=False, ext=True).reshape(vecs, n, 4)
    futures = [pool.submit(_job, f"ext 2^{log_n} x{vecs} vector {v} coordinate {k}", got[v, :, k], x[v, :, k], n, False, 1)
               for v in range(vecs) for k in range(4)]
    back = run(ta, got.reshape(-1), n, vecs, True, inplace=True, ext=True).reshape(vecs, n, 4)
    assert np.array_equal(back, x), "whole-batch round trip"
    settle(futures)
