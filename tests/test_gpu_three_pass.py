"""The three-pass plans, n = 2^23 .. 2^27 (split_passes, toyni_amd/csrc/ntt_plan.hpp), output for output against the oracle.

The rest of the GPU suite is dense up to n = 2^22 and then checks 2^24 and 2^27 through properties.  Here every size of the third
plan family -- splits (7,8,8), (8,8,8), (8,8,9), (8,9,9), (9,9,9) and the twiddle tables built for them -- goes through the device
entry points and EVERY output word is compared with oracle.* (bit-exact: integer path, no tolerance): plain and coset transforms,
the batches that move each pass between its tile widths, 512 MiB launches (the non-temporal twins), ragged chunks, the low-degree
extension through a 128- / 256- / 512-point zero-aware column pass, Ext (AoS) vectors, the domain table and the structured fold
on these contexts, and one transform over lanes of one device.  Each case asserts that the plan it ran had three passes.

The oracle is what costs: 30 s to a minute for one 2^27 transform on one thread.  It is a ctypes library (the GIL is released
during a call), so the transforms of a case are computed AND compared inside one pool of 8 threads; a result vector lives only
inside the worker that made it, which keeps a case under four vectors of 2^27 u64.

Wall time, measured on one MI355X host (16 CPUs): 302 s for this file; the whole `-m gpu` suite took 905 s with it and about
550 s without it (the suite as it was before this file).  That is more than a quarter of the earlier suite, and sampling inside
batches cannot change it -- no batch here has more than five transforms; the floor is the lone transforms of 2^26 and 2^27 that
every direction, size and zero fraction asks for (2^27: three tests of 27 - 32 s each, two oracle runs side by side at most under
the four-vector limit)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle
from dispatch_matrix import batches_for
from guarded import edge_residues
from oracle import P
from test_gpu_parity import DevBuf, ta  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

POOL_WORKERS = 8
DEAD = 0xDEADBEEF                      # >= p: no output word can equal it
CAP_LOG_ELEMS = 27                     # elements of one case
RANDOM_SHIFT = int(np.random.default_rng(0x3BA55).integers(2, P))     # the seeded random coset shift of this file


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(max_workers=POOL_WORKERS) as ex:
        yield ex


# ---------------------------------------------------------------- oracle side
def oracle_transform(x, n, inverse, shift):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    if shift == 1:
        return oracle.intt(x) if inverse else oracle.ntt(x)
    return oracle.domain_ifft(x, shift) if inverse else oracle.domain_fft(x, n, shift)


def oracle_lde(coeffs, n, shift):
    return oracle.domain_fft(np.ascontiguousarray(coeffs, dtype=np.uint64), n, shift)


def _job(label, got, fn, *args):
    """Runs in a pool thread: the oracle's vector is made, compared with every word of `got` and dropped here."""
    want = fn(*args)
    assert want.shape == got.shape, label
    if np.array_equal(got, want):
        return None
    bad = np.flatnonzero(got != want)
    return f"{label}: {bad.size} of {want.size} words differ from the oracle, first at index {int(bad[0])}"


def settle(futures):
    errors = [e for e in (f.result() for f in futures) if e]
    assert not errors, "\n".join(errors)


# ---------------------------------------------------------------- device side
def three_pass_ctx(ta, log_n, batch=1):
    ctx = ta.ntt.get_or_create_ctx(1 << log_n)
    assert ctx.passes_for(batch) == 3, f"2^{log_n} x {batch} no longer takes a three-pass plan"
    return ctx


def run_base(ta, x32, log_n, batch, inverse, inplace, shift=1):
    """One toyni_ntt_device / toyni_coset_ntt_device call on `batch` transforms; out of place: output prefilled, input checked."""
    n = 1 << log_n
    ctx = three_pass_ctx(ta, log_n, batch)
    a = DevBuf(ta, x32.nbytes, guard=4 * n)
    b = a if inplace else DevBuf(ta, x32.nbytes, guard=4 * n)
    try:
        a.upload(x32)
        if not inplace:
            b.upload(np.full(x32.size, DEAD, dtype=np.uint32))
        ctx.run_device(a.ptr, b.ptr, batch, inverse, shift=shift)
        ctx.synchronize()
        got = b.download(np.uint32, x32.size)
        if not inplace:
            assert np.array_equal(a.download(np.uint32, x32.size), x32), "out-of-place transform modified its input"
    finally:
        a.free()
        if b is not a:
            b.free()
    return got


def run_ext(ta, x, log_n, inverse, inplace, shift=1):
    """x: [vecs][n][4] u32 through toyni_ntt_ext_batch_device."""
    n, vecs = 1 << log_n, x.shape[0]
    ctx = three_pass_ctx(ta, log_n, 4 * vecs)
    a = DevBuf(ta, x.nbytes, guard=16 * n)
    b = a if inplace else DevBuf(ta, x.nbytes, guard=16 * n)
    try:
        a.upload(x)
        if not inplace:
            b.upload(np.full(x.size, DEAD, dtype=np.uint32))
        ctx.run_device_ext_batch(a.ptr, b.ptr, vecs, inverse, shift=shift)
        ctx.synchronize()
        got = b.download(np.uint32, x.size).reshape(x.shape)
        if not inplace:
            assert np.array_equal(a.download(np.uint32, x.size).reshape(x.shape), x), "out-of-place transform modified its input"
    finally:
        a.free()
        if b is not a:
            b.free()
    return got


def rows_vs_oracle(pool, label, x, got, n, rows, inverse, shift):
    return [pool.submit(_job, f"{label} transform {t}", got[t * n:(t + 1) * n], oracle_transform, x[t * n:(t + 1) * n], n, inverse, shift)
            for t in rows]


def ext_vs_oracle(pool, label, x, got, n, inverse, shift):
    """Every coordinate column of every vector ([vecs][n][4]) against the oracle's transform of that column."""
    return [pool.submit(_job, f"{label} vector {v} coordinate {k}", got[v, :, k], oracle_transform, x[v, :, k], n, inverse, shift)
            for v in range(x.shape[0]) for k in range(4)]


# ---------------------------------------------------------------- plain transforms, every output
@pytest.mark.parametrize("log_n", [23, 25, 26, 27])
def test_plain_forward_in_place_inverse_out_of_place(ta, pool, log_n):
    n = 1 << log_n
    x = oracle.splitmix(n, 0x3A55 + (log_n << 32))        # one u64 vector, shared by both oracle runs
    x32 = x.astype(np.uint32)
    fwd = run_base(ta, x32, log_n, 1, False, inplace=True)
    inv = run_base(ta, x32, log_n, 1, True, inplace=False)
    settle([pool.submit(_job, f"forward 2^{log_n}", fwd, oracle_transform, x, n, False, 1),
            pool.submit(_job, f"inverse 2^{log_n}", inv, oracle_transform, x, n, True, 1)])


def test_plain_2_27_field_edge_values(ta, pool):
    """Every edge class of the lazy reductions (tests/guarded.py) through the largest transform, forward, out of place."""
    log_n = 27
    n = 1 << log_n
    e32 = edge_residues(n, 0xED6E27)
    got = run_base(ta, e32, log_n, 1, False, inplace=False)
    settle([pool.submit(_job, "forward 2^27, edge residues", got, oracle_transform, e32, n, False, 1)])


# ---------------------------------------------------------------- coset transforms
@pytest.mark.parametrize("log_n,batch", [(22, 3), (23, 1), (25, 1), (26, 1)])     # 2^22: three transforms take the three-pass plan
def test_coset_forward_and_inverse(ta, pool, log_n, batch):
    n = 1 << log_n
    x32 = oracle.splitmix(n * batch, 0xC05E7 + log_n).astype(np.uint32)
    futures = []
    for shift in (7, RANDOM_SHIFT):
        for inverse in (False, True):
            inplace = (shift == 7) != inverse
            got = run_base(ta, x32, log_n, batch, inverse, inplace, shift=shift)
            futures += rows_vs_oracle(pool, f"coset 2^{log_n} x{batch} shift {shift} inverse={inverse}", x32, got, n, range(batch), inverse, shift)
    settle(futures)


# ---------------------------------------------------------------- batches and tile tiers
def _tier_cases():
    # the batches that carry each of the three passes over the 2^7, 2^9 and 2^12 32-wide-tile thresholds, a lone transform and three;
    # odd batches start with the inverse, so both directions meet the oracle in every tier
    cases = [(log_n, b, bool(b & 1)) for log_n in (23, 24) for b in batches_for(log_n, CAP_LOG_ELEMS)]
    # 512 MiB in one launch: the non-temporal twins under the default TOYNI_NT_MIN_BYTES
    return cases + [(25, 4, False), (26, 2, True)]


@pytest.mark.parametrize("log_n,batch,inverse_first", _tier_cases())
def test_batches_and_tile_tiers(ta, pool, log_n, batch, inverse_first):
    n = 1 << log_n
    assert log_n + (batch - 1).bit_length() <= CAP_LOG_ELEMS
    x32 = oracle.splitmix(n * batch, 0x71E5 + 64 * log_n + batch).astype(np.uint32)
    got = run_base(ta, x32, log_n, batch, inverse_first, inplace=False)
    rows = range(batch) if batch <= 4 else sorted({0, batch // 2, batch - 1})
    futures = rows_vs_oracle(pool, f"2^{log_n} x{batch} inverse={inverse_first}", x32, got, n, rows, inverse_first, 1)
    back = run_base(ta, got, log_n, batch, not inverse_first, inplace=True)      # the whole batch, the other direction
    assert np.array_equal(back, x32), "whole-batch round trip"
    settle(futures)


def test_tier_batches_cover_the_thresholds():
    # (no device) what batches_for hands the case above: at 2^23 the 128- and 256-point passes, at 2^24 the 256-point ones, each
    # below and at the 64-wide threshold of 2^12 32-wide tiles; every three-pass split contributes all of its pass sizes
    assert batches_for(23, CAP_LOG_ELEMS) == [1, 2, 3, 4] and batches_for(24, CAP_LOG_ELEMS) == [1, 2, 3]
    for log_n, logm in ((23, (7, 8, 8)), (24, (8, 8, 8)), (25, (8, 8, 9)), (26, (8, 9, 9)), (27, (9, 9, 9))):
        assert sum(logm) == log_n
        for m in logm:
            for lt in (7, 9, 12):
                b = 1 << max(0, lt + 5 + m - log_n)
                if log_n + (b - 1).bit_length() <= CAP_LOG_ELEMS:
                    assert b in batches_for(log_n, CAP_LOG_ELEMS), (log_n, m, lt)
                    assert (b << (log_n - m)) >> 5 >= 1 << lt


# ---------------------------------------------------------------- chunking
@pytest.mark.parametrize("log_n", [23, 24])
def test_ragged_chunks_equal_the_unchunked_call(ta, pool, log_n):
    n, batch = 1 << log_n, 5
    ctx = three_pass_ctx(ta, log_n, batch)
    x32 = oracle.splitmix(n * batch, 0xC4A2 + log_n).astype(np.uint32)
    whole = run_base(ta, x32, log_n, batch, False, inplace=True)
    futures = rows_vs_oracle(pool, f"2^{log_n} x{batch}", x32, whole, n, range(batch), False, 1)
    try:
        ctx.set_chunk(2 * n)                                   # 2 + 2 + 1 transforms
        for inplace in (True, False):
            assert np.array_equal(run_base(ta, x32, log_n, batch, False, inplace), whole), f"chunked forward, inplace={inplace}"
        for inplace in (True, False):
            assert np.array_equal(run_base(ta, whole, log_n, batch, True, inplace), x32), f"chunked inverse, inplace={inplace}"
    finally:
        ctx.set_chunk(0)
    settle(futures)


# ---------------------------------------------------------------- low-degree extension
def check_lde(ta, pool, log_n, z, batch, shift, ext=False):
    """toyni_lde_device / toyni_lde_ext_batch_device: every output against oracle.domain_fft(coeffs, n, shift) (per coordinate column
    for Ext vectors), the input untouched, and the same words from the plain transform of the hand-padded input.  Returns the oracle
    comparisons as futures: the caller settles them, so that the cases of one test share the pool."""
    n, q = 1 << log_n, 4 if ext else 1
    n_in = n >> z
    ctx = three_pass_ctx(ta, log_n, batch * q)
    assert ctx.passes == 3
    c = oracle.splitmix(n_in * batch * q, 0x1DE0 + 4096 * log_n + 64 * z + batch + (1 if ext else 0)).astype(np.uint32)
    a, o = DevBuf(ta, c.nbytes, guard=4 * n * q), DevBuf(ta, 4 * n * batch * q, guard=4 * n * q)
    try:
        a.upload(c)
        o.upload(np.full(n * batch * q, DEAD, dtype=np.uint32))
        (ctx.lde_ext_device if ext else ctx.lde_device)(a.ptr, o.ptr, batch, z, shift)
        ctx.synchronize()
        got = o.download(np.uint32, n * batch * q).reshape(batch, n, q)
        assert np.array_equal(a.download(np.uint32, c.size), c), "the extension modified its input"
    finally:
        a.free()
        o.free()
    cc = c.reshape(batch, n_in, q)
    label = f"lde{'_ext' if ext else ''} 2^{log_n} x{batch} blow-up 2^{z} shift {shift}"
    futures = [pool.submit(_job, f"{label} vector {t} coordinate {k}", got[t, :, k], oracle_lde, cc[t, :, k], n, shift)
               for t in range(batch) for k in range(q)]
    padded = np.zeros((batch, n, q), dtype=np.uint32)
    padded[:, :n_in] = cc
    if ext:
        same = run_ext(ta, padded, log_n, False, inplace=True, shift=shift)
    else:
        same = run_base(ta, padded.reshape(-1), log_n, batch, False, inplace=True, shift=shift).reshape(batch, n, q)
    assert np.array_equal(same, got), label + ": differs from the transform of the hand-padded input"
    return futures


def _m1_log(ta, log_n):
    return int(ta._lib.lib.toyni_ntt_ctx_first_pass_points(ta.ntt.get_or_create_ctx(1 << log_n).handle)).bit_length() - 1


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("z", [1, 2, 3, 4, 5])
def test_lde_2_23_every_zero_fraction(ta, pool, z, batch):
    settle(check_lde(ta, pool, 23, z, batch, 7 if (z + batch // 2) & 1 else RANDOM_SHIFT))     # each shift meets each batch and odd / even z


@pytest.mark.parametrize("log_n", [24, 25, 26])
def test_lde_2_24_to_2_26(ta, pool, log_n):
    futures = []
    for z in (1, 3, 5):
        futures += check_lde(ta, pool, log_n, z, 1, 7 if (z + log_n) & 2 else RANDOM_SHIFT)
    settle(futures)


@pytest.mark.parametrize("log_n,m1", [(23, 7), (25, 8)])
def test_lde_blowups_beyond_five_bits(ta, pool, log_n, m1):
    assert _m1_log(ta, log_n) == m1
    futures = check_lde(ta, pool, log_n, min(m1, 6), 1, 7)     # the LZ = 5 variant with its row guard
    settle(futures + check_lde(ta, pool, log_n, m1 + 1, 1, RANDOM_SHIFT))     # beyond the first pass: pad and transform


def test_lde_2_27(ta, pool):
    settle(check_lde(ta, pool, 27, 5, 1, 7))


# ---------------------------------------------------------------- Ext (AoS) vectors
@pytest.mark.parametrize("log_n,vecs", [(23, 1), (25, 1), (23, 2)])
def test_ext_vectors_every_coordinate(ta, pool, log_n, vecs):
    n = 1 << log_n
    x = oracle.splitmix(4 * n * vecs, 0xE87 + 64 * log_n + vecs).astype(np.uint32).reshape(vecs, n, 4)
    combos = [(False, 1), (True, 1), (False, 7), (True, RANDOM_SHIFT)] if vecs == 1 else [(False, RANDOM_SHIFT), (True, 1)]
    futures = []
    for i, (inverse, shift) in enumerate(combos):
        got = run_ext(ta, x, log_n, inverse, inplace=bool(i & 1), shift=shift)
        futures += ext_vs_oracle(pool, f"ext 2^{log_n} x{vecs} shift {shift} inverse={inverse}", x, got, n, inverse, shift)
        if i & 1:                                              # eight columns at a time: sixteen of 2^25 would be 4 GiB of oracle output
            settle(futures)
            futures = []
    settle(futures)


@pytest.mark.parametrize("log_n,z", [(23, 2), (23, 5), (25, 5)])
def test_ext_lde(ta, pool, log_n, z):
    settle(check_lde(ta, pool, log_n, z, 1, 7 if z == 5 else RANDOM_SHIFT, ext=True))


# ---------------------------------------------------------------- domain table and structured fold
@pytest.mark.parametrize("log_n,lowbits", [(23, 12), (25, 13), (26, 13)])
def test_domain_elements_and_fold_on_these_contexts(ta, pool, log_n, lowbits):
    """m = n >> k for k in {0, L-1, L, L+1}, L = the low-level bits of the context's two-level domain table: the three branches of
    sub_domain (the table itself, a compact subgroup level, the high level alone)."""
    assert lowbits == (log_n + 1) // 2                         # append_two_level
    ctx = ta.ntt.get_or_create_ctx(1 << log_n)
    assert ctx.passes == 3
    beta = 555555555
    futures = []
    for k in (0, lowbits - 1, lowbits, lowbits + 1):
        m = (1 << log_n) >> k
        shift = 7 if k & 1 else RANDOM_SHIFT
        buf = DevBuf(ta, 4 * m)
        try:
            buf.upload(np.full(m, DEAD, dtype=np.uint32))
            ctx.domain_elements_device(buf.ptr, m, shift)
            ctx.synchronize()
            got = buf.download(np.uint32, m)
        finally:
            buf.free()
        futures.append(pool.submit(_job, f"domain elements 2^{log_n} >> {k}", got, oracle.domain_elements, m, shift))
        evals = oracle.splitmix(m, 0xF01D + 64 * log_n + k)
        e32 = evals.astype(np.uint32)
        a, o = DevBuf(ta, 4 * m), DevBuf(ta, 2 * m)
        try:
            a.upload(e32)
            o.upload(np.full(m // 2, DEAD, dtype=np.uint32))
            ta.fri_fold_device(ctx, a.ptr, o.ptr, m, beta, shift)
            ctx.synchronize()
            folded = o.download(np.uint32, m // 2)
            assert np.array_equal(a.download(np.uint32, m), e32), "the fold modified its input"
        finally:
            a.free()
            o.free()
        futures.append(pool.submit(_job, f"fold 2^{log_n} >> {k}", folded,
                                   lambda e, mm, s: oracle.fri_fold(e, oracle.domain_elements(mm, s), beta), evals, m, shift))
    settle(futures)


# ---------------------------------------------------------------- one transform over lanes of one device
@pytest.mark.parametrize("log_n,lanes,m1", [(23, 4, 1 << 7), (25, 8, 1 << 8), (26, 2, 1 << 8)])
def test_slab_lanes_natural_order(ta, pool, log_n, lanes, m1):
    n = 1 << log_n
    assert int(ta._lib.lib.toyni_first_pass_points(n)) == m1
    assert ta.ntt.get_or_create_ctx(n).passes == 3
    x = oracle.splitmix(n, 0x51AB + 64 * log_n + lanes)
    fwd, inv = x.copy(), x.copy()
    ta.ntt_slab_multi_gpu_host(fwd, [0] * lanes)
    ta.ntt_slab_multi_gpu_host(inv, [0] * lanes, inverse=True)
    settle([pool.submit(_job, f"slab forward 2^{log_n} over {lanes} lanes", fwd, oracle_transform, x, n, False, 1),
            pool.submit(_job, f"slab inverse 2^{log_n} over {lanes} lanes", inv, oracle_transform, x, n, True, 1)])
