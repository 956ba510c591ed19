"""Every device entry point between guard bands, fed field-edge values (tests/guarded.py).

Each case asserts
  (a) both guards of every buffer are intact after the call has been synchronised;
  (b) every output word is canonical -- outputs are pre-filled with 0xA5A5A5A5 >= p, so a word the call skips fails here;
  (c) the output equals the oracle bit for bit (all of it, or first / middle / last transform of a large batch);
  (d) out-of-place calls leave their inputs byte-identical;
  (e) the case runs a second time with seeded random canonical words in the guards around its inputs, and gives identical
      outputs: a read outside the inputs (past an LDE's coefficients, past xs[m/2), past the trace) changes the result.
Zero-size work writes nothing, and arguments the library refuses leave the output payload and its guards untouched.  Batches come
from the dispatch seams that tests/dispatch_matrix.py walks (batches_for: the tile-width tiers of every pass), LDE blow-ups from the
first pass's size (toyni_ntt_ctx_first_pass_points); oracle work stays under ~2^23 elements per case, like tests/test_gpu_fuzz.py."""
import ctypes

import numpy as np
import pytest

import oracle
from dispatch_matrix import batches_for
from guarded import GUARD_MIN, Guarded, HostMem, edge_residues, edge_u64, memory_of, reduce_u64
from harness import ref_prover
from oracle import P

pytestmark = pytest.mark.gpu

E_ODD, E_ZERO_INV, E_RANGE = 10003, 10005, 10006
OFFSETS = (0, 4, 8, 12)
CAP_LOG = 23


@pytest.fixture(scope="module")
def ta():
    import __graft_entry__ as entry
    entry.build_hip()
    import toyni_amd
    assert toyni_amd.gpu_available(), "GPU tests need a device"
    return toyni_amd


def guard_for(nbytes):
    return min(max(nbytes, GUARD_MIN), 32 << 20)


class Case:
    """The buffers of one call.  run(call) performs (a), (b), (d), (e) and returns the outputs of the first run for (c)."""

    def __init__(self, mem, name):
        self.mem, self.name = memory_of(mem), name
        self.ins, self.outs, self.inouts = [], [], []
        self._seed = 0

    def _new(self, nbytes, offset, word, guard):
        self._seed += 1
        return Guarded(self.mem, nbytes, offset=offset, word=word, guard=guard if guard is not None else guard_for(nbytes), seed=self._seed)

    def inp(self, arr, offset=0, word=4, guard=None):
        arr = np.ascontiguousarray(arr)
        g = self._new(max(arr.nbytes, 0), offset, word, guard)
        self.ins.append((g, arr))
        return g

    def out(self, nbytes, offset=0, word=4, guard=None):
        g = self._new(nbytes, offset, word, guard)
        self.outs.append(g)
        return g

    def inout(self, arr, offset=0, word=4, guard=None):
        arr = np.ascontiguousarray(arr)
        g = self._new(arr.nbytes, offset, word, guard)
        self.inouts.append((g, arr))
        return g

    def _prepare(self, pattern):
        for g, host in self.ins:
            g.refill(pattern)
            g.upload(host)
        for g, host in self.inouts:
            g.fill_sentinel()
            g.refill(pattern)
            g.upload(host)
        for g in self.outs:
            g.fill_sentinel()

    def run(self, call, canonical=True, expect=0, patterns=("sentinel", "random")):
        results = []
        for pattern in patterns:
            self._prepare(pattern)
            rc = call()
            assert rc == expect, f"{self.name}: status {rc}, expected {expect}"
            self.mem.sync()
            for k, (g, _) in enumerate(self.ins):
                g.check(f"{self.name}: input {k}")
            for k, g in enumerate(self.outs + [g for g, _ in self.inouts]):
                g.check(f"{self.name}: output {k}")
            for k, (g, host) in enumerate(self.ins):                              # (d)
                got = g.download(np.uint8, host.nbytes)
                assert (got == host.view(np.uint8).reshape(-1)).all(), f"{self.name}: input {k} changed by an out-of-place call"
            results.append([g.download() for g in self.outs] + [g.download() for g, _ in self.inouts])
        if len(results) == 2:                                                     # (e)
            for k, (a, b) in enumerate(zip(*results)):
                bad = np.flatnonzero(a != b)
                assert not bad.size, f"{self.name}: output {k} depends on bytes outside the inputs (first at word {bad[0]})"
        if canonical:                                                             # (b)
            for k, o in enumerate(results[0]):
                if o.dtype != np.uint8:
                    bad = np.flatnonzero(o >= P)
                    assert not bad.size, f"{self.name}: output {k} word {bad[0]} = {o[bad[0]]:#x} not canonical (unwritten?)"
        return results[0]

    def untouched(self):
        """After a refused call: every output payload still the sentinel, inputs as uploaded."""
        for k, g in enumerate(self.outs):
            assert (g.download(np.uint8) == 0xA5).all(), f"{self.name}: refused call wrote output {k}"
        for g, host in self.inouts:
            assert (g.download(np.uint8, host.nbytes) == host.view(np.uint8).reshape(-1)).all(), f"{self.name}: refused call wrote"

    def free(self):
        err = None
        for g in [g for g, _ in self.ins] + self.outs + [g for g, _ in self.inouts]:
            try:
                g.free()
            except AssertionError as e:
                err = err or e
        if err:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.size == want.size, what
    bad = np.flatnonzero(got.astype(np.uint64) != want.astype(np.uint64))
    assert not bad.size, f"{what}: {bad.size} words differ from the oracle, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def samples(batch):
    return sorted({0, batch // 2, batch - 1})


def ctx_of(ta, log_n):
    return ta.ntt.get_or_create_ctx(1 << log_n)


def seam_batches(log_n):
    """Batches at the tile-width seams of an n-point plan (batches_for), capped at 2^CAP_LOG elements, plus one ragged batch."""
    bs = [b for b in batches_for(log_n, CAP_LOG) if log_n + (b - 1).bit_length() <= CAP_LOG]
    if log_n >= 21:
        bs = [1, max(bs)]
    return sorted(set(bs + [3 if log_n + 2 <= CAP_LOG else 1]))


SHIFTS = (1, 7, P - 1)
NTT_SIZES = (10, 11, 12, 13, 16, 20, 21, 22)


# ---------------------------------------------------------------- base-field transforms
@pytest.mark.parametrize("log_n", NTT_SIZES)
def test_ntt_device_seams(ta, log_n):
    n = 1 << log_n
    ctx = ctx_of(ta, log_n)
    lib = ta._lib.lib
    k = 0
    for batch in seam_batches(log_n):
        x = edge_residues(n * batch, 1000 * log_n + batch)
        for inverse in (0, 1):
            shift, off, inplace = SHIFTS[k % 3], OFFSETS[k % 4], (k + k // 2) % 2 == 1   # both directions both ways
            k += 1
            name = f"ntt 2^{log_n} x{batch} {'inv' if inverse else 'fwd'} shift {shift} off {off} {'in' if inplace else 'out of'} place"
            with Case(ta, name) as c:
                if inplace:
                    a = c.inout(x, off)
                    b = a
                else:
                    a, b = c.inp(x, off), c.out(x.nbytes, (off + 4) % 16)
                if shift == 1:
                    call = lambda: lib.toyni_ntt_device(ctx.handle, a.ptr, b.ptr, batch, inverse, None)
                else:
                    call = lambda: lib.toyni_coset_ntt_device(ctx.handle, a.ptr, b.ptr, batch, shift, inverse, None)
                y = c.run(call)[0]
            for t in samples(batch):
                xt = x[t * n:(t + 1) * n].astype(np.uint64)
                want = oracle.domain_ifft(xt, shift) if inverse else oracle.domain_fft(xt, n, shift)
                same(y[t * n:(t + 1) * n], want, f"{name}: transform {t}")


@pytest.mark.parametrize("log_n", [1, 10, 12, 13, 21])
def test_ntt_device_u64_noncanonical_inputs(ta, log_n):
    n, batch = 1 << log_n, 3 if log_n < 21 else 1
    ctx = ctx_of(ta, log_n)
    x = edge_u64(n * batch, 77 + log_n)
    for inverse in (0, 1):
        with Case(ta, f"u64 2^{log_n} x{batch} inv={inverse}") as c:
            a = c.inout(x, 8 * (inverse + 1) % 16, word=8)
            y = c.run(lambda: ta._lib.lib.toyni_ntt_device_u64(ctx.handle, a.ptr, batch, inverse, None))[0]
        for t in samples(batch):
            xt = reduce_u64(x[t * n:(t + 1) * n])
            same(y[t * n:(t + 1) * n], oracle.intt(xt) if inverse else oracle.ntt(xt), f"u64 2^{log_n} transform {t}")


# ---------------------------------------------------------------- Ext transforms and low-degree extensions
@pytest.mark.parametrize("log_n", [1, 10, 11, 12, 13, 16, 20])
def test_ext_transforms(ta, log_n):
    n = 1 << log_n
    ctx = ctx_of(ta, log_n)
    lib = ta._lib.lib
    k = 0
    for batch in (1, 3):
        x = edge_residues(4 * n * batch, 3000 + log_n + batch)
        for inverse in (0, 1):
            shift, off, inplace = SHIFTS[k % 3], OFFSETS[(k + 1) % 4], (k + k // 2) % 2 == 0
            k += 1
            name = f"ext 2^{log_n} x{batch} inv={inverse} shift {shift} off {off} inplace={inplace}"
            with Case(ta, name) as c:
                if inplace:
                    a = b = c.inout(x, off)
                else:
                    a, b = c.inp(x, off), c.out(x.nbytes, 12 - off)
                y = c.run(lambda: lib.toyni_ntt_ext_batch_device(ctx.handle, a.ptr, b.ptr, batch, shift, inverse, None))[0]
            xx, yy = x.reshape(batch, n, 4).astype(np.uint64), y.reshape(batch, n, 4)
            for t in samples(batch):
                for q in range(4):
                    want = oracle.domain_ifft(xx[t, :, q], shift) if inverse else oracle.domain_fft(xx[t, :, q], n, shift)
                    same(yy[t, :, q], want, f"{name}: vector {t} coordinate {q}")
    # the single-vector in-place form
    x = edge_residues(4 * n, 3100 + log_n)
    with Case(ta, f"ext single 2^{log_n}") as c:
        a = c.inout(x, 4)
        y = c.run(lambda: lib.toyni_ntt_ext_device(ctx.handle, a.ptr, P - 1, 0, None))[0].reshape(n, 4)
    for q in range(4):
        same(y[:, q], oracle.domain_fft(x.reshape(n, 4)[:, q].astype(np.uint64), n, P - 1), f"ext single 2^{log_n} coordinate {q}")


def lde_blowups(ta, log_n):
    ctx = ctx_of(ta, log_n)
    m1p = int(ta._lib.lib.toyni_ntt_ctx_first_pass_points(ctx.handle))
    m1 = m1p.bit_length() - 1 if m1p else 0
    zs = list(range(1, min(5, m1) + 1)) if m1 else [1, 2]
    zs.append((m1 + 1) if m1 else min(3, log_n))            # past the first pass (or a single-pass size): padding materialised
    return sorted(set(z for z in zs if z <= log_n))


@pytest.mark.parametrize("log_n", [4, 10, 12, 16, 20, 21, 22])
def test_lde_reads_only_the_coefficients(ta, log_n):
    """The coefficients are followed by random canonical words in the second run: the padding must be implied, not read."""
    n = 1 << log_n
    ctx = ctx_of(ta, log_n)
    lib = ta._lib.lib
    for k, z in enumerate(lde_blowups(ta, log_n)):
        n_in = n >> z
        for ext in (False, True):
            if ext and log_n > 20:
                continue
            q = 4 if ext else 1
            batch = 3 if log_n <= 16 else 1
            shift, off = SHIFTS[(k + ext) % 3], OFFSETS[(k + 2 * ext) % 4]
            cf = edge_residues(n_in * batch * q, 5000 + 10 * log_n + z)
            name = f"lde{'_ext' if ext else ''} 2^{log_n} x{batch} blow-up 2^{z} shift {shift} off {off}"
            with Case(ta, name) as c:
                a, b = c.inp(cf, off), c.out(4 * n * batch * q, (16 - off) % 16)
                if ext:
                    call = lambda: lib.toyni_lde_ext_batch_device(ctx.handle, a.ptr, b.ptr, batch, z, shift, None)
                else:
                    call = lambda: lib.toyni_lde_device(ctx.handle, a.ptr, b.ptr, batch, z, shift, None)
                y = c.run(call)[0].reshape(batch, n, q)
            cc = cf.reshape(batch, n_in, q).astype(np.uint64)
            for t in samples(batch):
                for j in (range(4) if ext and t == 0 else [t % q]):
                    same(y[t, :, j], oracle.domain_fft(cc[t, :, j], n, shift), f"{name}: vector {t} coordinate {j}")
        if log_n <= 12 and k == 0:
            x = edge_residues(n_in * 4, 5500 + log_n)
            with Case(ta, f"lde_ext single 2^{log_n}") as c:
                a, b = c.inp(x, 8), c.out(16 * n, 4)
                y = c.run(lambda: lib.toyni_lde_ext_device(ctx.handle, a.ptr, b.ptr, z, 7, None))[0].reshape(n, 4)
            for j in range(4):
                same(y[:, j], oracle.domain_fft(x.reshape(n_in, 4)[:, j].astype(np.uint64), n, 7), f"lde_ext single coordinate {j}")


def test_domain_elements(ta):
    ctx = ctx_of(ta, 12)
    for m, off in ((1, 4), (2, 8), (64, 12), (1024, 0), (4096, 4)):
        for shift in (1, P - 1):
            with Case(ta, f"domain m={m} shift {shift}") as c:
                o = c.out(4 * m, off)
                y = c.run(lambda: ta._lib.lib.toyni_domain_elements_device(ctx.handle, o.ptr, m, shift, None))[0]
            same(y, oracle.domain_elements(m, shift), f"domain elements m={m} shift {shift}")


# ---------------------------------------------------------------- folds
STRUCT_M = (2, 8, 64, 1 << 12, 1 << 19)
BETAS = (0, 1, P - 1, 424242)


@pytest.mark.parametrize("m", STRUCT_M)
def test_fold_structured(ta, m):
    ctx = ctx_of(ta, 20)
    for k, off in enumerate((0, 4)):
        beta, x0 = BETAS[(k + m.bit_length()) % 4], (P - 1, 7)[k]
        e = edge_residues(m, 600 + m + k)
        name = f"fold m={m} beta {beta} x0 {x0} off {off}"
        with Case(ta, name) as c:
            a, o = c.inp(e, off), c.out(2 * m, off)
            y = c.run(lambda: ta._lib.lib.toyni_fri_fold_device(ctx.handle, a.ptr, o.ptr, m, beta, x0, None))[0]
        same(y, oracle.fri_fold(e.astype(np.uint64), oracle.domain_elements(m, x0), beta), name)


@pytest.mark.parametrize("log_n,off", [(3, 0), (12, 4), (16, 0)])
def test_fold_layers_back_to_back(ta, log_n, off):
    n = 1 << log_n
    ctx = ctx_of(ta, log_n)
    betas = np.array([BETAS[k % 4] for k in range(log_n)], dtype=np.uint32)
    e = edge_residues(n, 700 + log_n)
    total = n - 1                                           # n/2 + n/4 + ... + 1
    with Case(ta, f"fold layers 2^{log_n}") as c:
        a, o = c.inp(e, off), c.out(4 * total, off)          # the guard sits right after the last layer
        y = c.run(lambda: ta._lib.lib.toyni_fri_fold_layers_device(ctx.handle, a.ptr, o.ptr, betas.ctypes.data, log_n, P - 1, None))[0]
    same(y, np.concatenate(oracle.fri_fold_layers(e.astype(np.uint64), P - 1, betas.astype(np.uint64))), f"fold layers 2^{log_n}")


def fold_xs_want(e, xs, beta):
    m = e.size
    x1 = np.where(xs == 0, 1, xs).astype(np.uint64)
    want = oracle.fri_fold(e.astype(np.uint64), x1, beta)
    for i in np.flatnonzero(xs == 0):   # x^-1 := 0: only the average survives
        want[i] = oracle.bb_mul(oracle.bb_add(int(e[i]), int(e[i + m // 2])), (P + 1) // 2)
    return want


XS_M = [(2, 0), (6, 4), (8, 0), (1024 + 8, 12), (1 << 19, 0), (1 << 19, 4), ((1 << 19) + 4, 0)]


@pytest.mark.parametrize("m,off", XS_M)
def test_fold_xs_reads_only_half_the_points(ta, m, off):
    """xs holds exactly m/2 words with the guard right after them; 2^19 at offset 4 must take fri_fold_xs_kernel, 2^19 + 4 the
    non-xs16 path at a large size."""
    beta = BETAS[(m + off) % 4]
    e = edge_residues(m, 800 + m)
    xs = edge_residues(m // 2, 900 + m)
    xs[xs == 0] = 1
    xs[-1] = 0                                               # a zero point in the tail
    if m >= 8:
        xs[m // 2 - 3] = P - 1
    name = f"fold_xs m={m} off {off} beta {beta}"
    with Case(ta, name) as c:
        a, x, o = c.inp(e, off), c.inp(xs, off), c.out(2 * m, off)
        y = c.run(lambda: ta._lib.lib.toyni_fri_fold_xs_device(a.ptr, x.ptr, o.ptr, m, beta, None))[0]
    same(y, fold_xs_want(e, xs, beta), name)


EXT_BETAS = ((0, 0, 0, 0), (P - 1, P - 1, P - 1, P - 1), (0, 0, 0, 1), (5, P - 2, 1, 1 << 27))


@pytest.mark.parametrize("m", [2, 8, 1024, 1 << 16])
def test_fold_ext(ta, m):
    ctx = ctx_of(ta, 20)
    for k, beta in enumerate(EXT_BETAS):
        b = np.array(beta, dtype=np.uint32)
        e = edge_residues(4 * m, 1100 + m + k)
        x0 = (P - 1, 7)[k % 2]
        name = f"fold_ext m={m} beta {beta} x0 {x0}"
        with Case(ta, name) as c:
            a, o = c.inp(e, 0), c.out(8 * m, 0)
            y = c.run(lambda: ta._lib.lib.toyni_fri_fold_ext_device(ctx.handle, a.ptr, o.ptr, m, b.ctypes.data, x0, None))[0]
        same(y, oracle.fri_fold_ext(e.astype(np.uint64), oracle.domain_elements(m, x0), b.astype(np.uint64)), name)
        xs = edge_residues(m // 2, 1200 + m + k)
        xs[xs == 0] = P - 1
        name = f"fold_ext_xs m={m} beta {beta}"
        with Case(ta, name) as c:
            a, x, o = c.inp(e, 0), c.inp(xs, 4 * (k % 4)), c.out(8 * m, 0)
            y = c.run(lambda: ta._lib.lib.toyni_fri_fold_ext_xs_device(a.ptr, x.ptr, o.ptr, m, b.ctypes.data, None))[0]
        same(y, oracle.fri_fold_ext(e.astype(np.uint64), xs.astype(np.uint64), b.astype(np.uint64)), name)


@pytest.mark.parametrize("m", [2, 6, 1032])
def test_fold_host_forms_with_host_guards(ta, m):
    """The host-slice folds write exactly len/2 (Ext: 4 len/2) u64 elements of a larger array and read nothing past their inputs."""
    mem = HostMem()
    lib = ta._lib.lib
    e = edge_u64(m, 1300 + m)
    xs = reduce_u64(edge_u64(m // 2, 1400 + m))
    xs[xs == 0] = 3
    with Case(mem, f"fold_host m={m}") as c:
        a, x, o = c.inp(e, word=8), c.inp(xs, word=8), c.out(4 * m, word=8)
        y = c.run(lambda: lib.toyni_fri_fold_host(o.ptr, a.ptr, m, x.ptr, P - 1))[0]
    same(y, oracle.fri_fold(reduce_u64(e), xs, P - 1), f"fold_host m={m}")
    ee = edge_u64(4 * m, 1500 + m)
    beta = np.array([P - 1, 0, 1, P - 1], dtype=np.uint64)
    with Case(mem, f"fold_ext_host m={m}") as c:
        a, x, o = c.inp(ee, word=8), c.inp(xs, word=8), c.out(16 * m, word=8)
        y = c.run(lambda: lib.toyni_fri_fold_ext_host(o.ptr, a.ptr, m, x.ptr, beta.ctypes.data))[0]
    same(y, oracle.fri_fold_ext(reduce_u64(ee), xs, beta), f"fold_ext_host m={m}")


# ---------------------------------------------------------------- Merkle, fold rounds, openings
MERKLE_N = (1, 2, 3, 5, 33, 1000, (1 << 12) + 1)


@pytest.mark.parametrize("n", MERKLE_N)
def test_merkle_commit(ta, n):
    lib = ta._lib.lib
    digests = int(lib.toyni_merkle_total_digests(n))
    vals = edge_residues(n, 1600 + n)
    salts = np.random.default_rng(n).integers(0, 256, (n, 16), dtype=np.uint8)
    for salted in (False, True):
        want = np.concatenate(oracle.merkle_commit_values(vals.astype(np.uint64), salts if salted else None)).reshape(-1)
        with Case(ta, f"merkle n={n} salted={salted}") as c:
            v = c.inp(vals, 4 if n & 1 else 0)
            s = c.inp(salts.reshape(-1), word=1) if salted else None
            lv = c.out(32 * digests, word=1)
            y = c.run(lambda: lib.toyni_merkle_commit_device(v.ptr, s.ptr if s else None, n, lv.ptr, None))[0]
        same(y, want, f"merkle commit n={n} salted={salted}")
        with Case(HostMem(), f"merkle host n={n}") as c:
            v = c.inp(vals.astype(np.uint64), word=8)
            s = c.inp(salts.reshape(-1), word=1) if salted else None
            lv = c.out(32 * digests, word=1)
            y = c.run(lambda: lib.toyni_merkle_commit_host(v.ptr, s.ptr if s else None, n, lv.ptr))[0]
        same(y, want, f"merkle commit host n={n} salted={salted}")


@pytest.mark.parametrize("m", [2, 64, 1 << 12])
def test_fold_commit_round(ta, m):
    ctx = ctx_of(ta, 16)
    lib = ta._lib.lib
    h = m // 2
    e = edge_residues(m, 1700 + m)
    salts = np.random.default_rng(m).integers(0, 256, (h, 16), dtype=np.uint8)
    folded = oracle.fri_fold(e.astype(np.uint64), oracle.domain_elements(m, P - 1), P - 1)
    levels = np.concatenate(oracle.merkle_commit_values(folded, salts)).reshape(-1)
    with Case(ta, f"fold commit m={m}") as c:
        a, o = c.inp(e, 4), c.out(4 * h, 8)
        s = c.inp(salts.reshape(-1), word=1)
        lv = c.out(32 * int(lib.toyni_merkle_total_digests(h)), word=1)
        y, yl = c.run(lambda: lib.toyni_fri_fold_commit_device(ctx.handle, a.ptr, o.ptr, m, P - 1, P - 1, s.ptr, lv.ptr, None))
    same(y, folded, f"fold commit m={m}: layer")
    same(yl, levels, f"fold commit m={m}: tree")


def test_commit_phase(ta):
    """The whole fold loop: layers, trees and roots each end exactly where the header says."""
    lib = ta._lib.lib
    m0, final = 1 << 10, 4
    ctx = ctx_of(ta, 10)
    e = edge_residues(m0, 1800)
    sizes = []
    m = m0
    while m > final:
        m //= 2
        sizes.append(m)
    nsalt = sum(sizes[:-1])
    salts = np.random.default_rng(5).integers(0, 256, (nsalt, 16), dtype=np.uint8)
    betas = [P - 1, 0, 1, 12345, P - 2, 7, 9, 11]
    x0 = 7
    layers, trees, cur, x, soff = [], [], e.astype(np.uint64), x0, 0
    for k, h in enumerate(sizes):
        f = oracle.fri_fold(cur, oracle.domain_elements(2 * h, x), betas[k])
        s = salts[soff:soff + h] if k < len(sizes) - 1 else None
        soff += h if s is not None else 0
        layers.append(f)
        trees.append(np.concatenate(oracle.merkle_commit_values(f, s)).reshape(-1))
        cur, x = f, oracle.bb_mul(x, x)
    nlev = sum(t.size for t in trees)

    @ta._lib.FRI_CHALLENGE_FN
    def challenge(user, rnd, root, beta_out):
        if beta_out:
            beta_out[0] = betas[rnd]
        return 0

    rounds = ctypes.c_uint(0)
    with Case(ta, "commit phase") as c:
        a, s = c.inp(e, 4), c.inp(salts.reshape(-1), word=1)
        lo, lv = c.out(4 * sum(sizes), 4), c.out(nlev, word=1)
        hr = Guarded(HostMem(), 32 * len(sizes), word=1)
        try:
            def call():
                hr.fill_sentinel()
                return lib.toyni_fri_commit_phase_device(ctx.handle, a.ptr, m0, x0, final, s.ptr, challenge, None, lo.ptr, lv.ptr, hr.ptr,
                                                         ctypes.byref(rounds), None)
            y, yl = c.run(call)
            hr.check("h_roots")
            got_roots = hr.download(np.uint8)
        finally:
            hr.free()
    assert rounds.value == len(sizes)
    same(y, np.concatenate(layers), "commit phase: layers")
    same(yl, np.concatenate(trees), "commit phase: trees")
    same(got_roots, np.concatenate([t[-32:] for t in trees]), "commit phase: roots")


@pytest.mark.parametrize("n", [5, 33, 1000])
@pytest.mark.parametrize("nidx", [1, 3, 33])
def test_merkle_openings(ta, n, nidx):
    lib = ta._lib.lib
    vals = edge_residues(n, 1900 + n)
    salts = np.random.default_rng(n).integers(0, 256, (n, 16), dtype=np.uint8)
    levels = oracle.merkle_commit_values(vals.astype(np.uint64), salts)
    flat = np.concatenate(levels).reshape(-1)
    idx = np.array((list(range(n)) * 40)[:nidx] if nidx > n else np.linspace(0, n - 1, nidx).astype(int), dtype=np.uint32)
    idx[-1] = n - 1
    rec = int(lib.toyni_merkle_open_record_bytes(n))
    _, want = ref_prover.serialize_openings(levels, vals.astype(np.uint64), salts, idx.tolist())
    with Case(ta, f"open n={n} nidx={nidx}") as c:
        lv, v, s, ix = c.inp(flat, word=1), c.inp(vals, 4), c.inp(salts.reshape(-1), word=1), c.inp(idx, 12)
        o = c.out(nidx * rec, 8, word=1)
        y = c.run(lambda: lib.toyni_merkle_open_device(lv.ptr, n, v.ptr, s.ptr, ix.ptr, nidx, o.ptr, None))[0]
    same(y, want, f"openings n={n} nidx={nidx}")
    # the grouped form: two trees in one launch
    with Case(ta, f"open groups n={n} nidx={nidx}") as c:
        lv, v, s, ix = c.inp(flat, word=1), c.inp(vals), c.inp(salts.reshape(-1), word=1), c.inp(idx)
        o1, o2 = c.out(nidx * rec, 0, word=1), c.out(nidx * rec, 8, word=1)
        G = OpenGroup * 2
        g = G(OpenGroup(lv.ptr, n, v.ptr, s.ptr, ix.ptr, nidx, o1.ptr), OpenGroup(lv.ptr, n, v.ptr, None, ix.ptr, nidx, o2.ptr))
        y1, y2 = c.run(lambda: lib.toyni_merkle_open_groups_device(ctypes.addressof(g), 2, None))
    same(y1, want, f"open groups n={n}: salted tree")
    _, want_unsalted_salt = ref_prover.serialize_openings(levels, vals.astype(np.uint64), None, idx.tolist())
    same(y2, want_unsalted_salt, f"open groups n={n}: NULL salts")


class OpenGroup(ctypes.Structure):
    _fields_ = [("d_levels", ctypes.c_void_p), ("n", ctypes.c_size_t), ("d_values", ctypes.c_void_p), ("d_salts", ctypes.c_void_p),
                ("d_indices", ctypes.c_void_p), ("nidx", ctypes.c_size_t), ("d_out", ctypes.c_void_p)]


# ---------------------------------------------------------------- prover steps
def deep_point(i, trace, q, N, B, shift, z, ood):
    t_z, t_gz, t_ggz, q_z = ood
    x = shift * pow(oracle.root_of_unity(N.bit_length() - 1), i, P) % P
    num = ((int(q[i]) - q_z) + (int(trace[(i + 2 * B) % N]) - t_ggz) + (int(trace[(i + B) % N]) - t_gz) + (int(trace[i]) - t_z)) % P
    d = (x - z) % P
    return 0 if d == 0 else num * pow(d, P - 2, P) % P


@pytest.mark.parametrize("log_N,log_blowup", [(6, 1), (12, 2), (12, 3), (16, 2)])
def test_quotient_and_deep(ta, log_N, log_blowup):
    N = 1 << log_N
    n, B = N >> log_blowup, 1 << log_blowup
    ctx = ctx_of(ta, log_N)
    lib = ta._lib.lib
    lde = edge_residues(N, 2000 + log_N)
    for k, (shift, off) in enumerate(((7, 0), (P - 2, 4))):
        c_want, q_want = oracle.fib_quotient(lde.astype(np.uint64), n, shift)
        for with_c in (True, False):
            name = f"quotient 2^{log_N} B={B} shift {shift} off {off} c={with_c}"
            with Case(ta, name) as c:
                t = c.inp(lde, off)
                co = c.out(4 * N, off) if with_c else None
                qo = c.out(4 * N, off)
                outs = c.run(lambda: lib.toyni_fib_quotient_device(ctx.handle, t.ptr, co.ptr if co else None, qo.ptr, log_blowup, shift, None))
            if with_c:
                same(outs[0], c_want, name + ": c")
            same(outs[-1], q_want, name + ": q")
        ood = (P - 1, P - 1, 0, P - 1)
        z = 1234567
        name = f"deep 2^{log_N} shift {shift}"
        with Case(ta, name) as c:
            t, q, o = c.inp(lde, off), c.inp(q_want.astype(np.uint32), (off + 8) % 16), c.out(4 * N, off)
            oodv = np.array(ood, dtype=np.uint32)
            y = c.run(lambda: lib.toyni_fib_deep_device(ctx.handle, t.ptr, q.ptr, o.ptr, log_blowup, shift, z, oodv.ctypes.data, None))[0]
        same(y, oracle.fib_deep(lde.astype(np.uint64), q_want, n, shift, z, *ood), name)
        # z on the coset: x_0 and x_{N-1} -- that point alone is 0, every other point as the formula says
        w = oracle.root_of_unity(log_N)
        for zi in (0, N - 1):
            zz = shift * pow(w, zi, P) % P
            with Case(ta, f"deep z = x_{zi}") as c:
                t, q, o = c.inp(lde), c.inp(q_want.astype(np.uint32)), c.out(4 * N)
                y = c.run(lambda: lib.toyni_fib_deep_device(ctx.handle, t.ptr, q.ptr, o.ptr, log_blowup, shift, zz, oodv.ctypes.data, None))[0]
            assert y[zi] == 0, f"deep z = x_{zi}: that point must be 0"
            for i in sorted({0, 1, zi, N // 2, N - 2, N - 1, (zi + 1) % N}):
                assert int(y[i]) == deep_point(i, lde, q_want, N, B, shift, zz, ood), f"deep z = x_{zi}: point {i}"


def test_quotient_refuses_a_vanishing_coset_without_writing(ta):
    """shift = p-1: (p-1)^n = 1, Z_H vanishes on the whole coset -- TOYNI_E_ZERO_INVERSE, and nothing written."""
    N = 1 << 10
    ctx = ctx_of(ta, 10)
    lde = edge_residues(N, 2100)
    with Case(ta, "quotient shift p-1") as c:
        t, co, qo = c.inp(lde), c.out(4 * N), c.out(4 * N)
        c.run(lambda: ta._lib.lib.toyni_fib_quotient_device(ctx.handle, t.ptr, co.ptr, qo.ptr, 2, P - 1, None), canonical=False,
              expect=E_ZERO_INV, patterns=("sentinel",))
        c.untouched()


@pytest.mark.parametrize("ncoeffs", [1, 1000, 70001])
def test_poly_eval(ta, ncoeffs):
    ctx = ctx_of(ta, 12)
    cf = edge_residues(ncoeffs, 2200 + ncoeffs)
    for npoints in (1, 2, 3, 4):
        pts = np.array([P - 1, 0, 1 << 27, 1234567][:npoints], dtype=np.uint32)
        with Case(ta, f"poly_eval {ncoeffs} x{npoints}") as c:
            a, o = c.inp(cf, 4 * npoints % 16), c.out(4 * npoints, 4)     # the guard starts right after npoints words
            y = c.run(lambda: ta._lib.lib.toyni_poly_eval_device(ctx.handle, a.ptr, ncoeffs, pts.ctypes.data, npoints, o.ptr, None))[0]
        same(y, [oracle.poly_eval(cf.astype(np.uint64), int(x)) for x in pts], f"poly_eval {ncoeffs} x{npoints}")


# ---------------------------------------------------------------- plumbing
@pytest.mark.parametrize("count", [1, 255, 257, 1000, (1 << 16) + 3])
def test_narrow_widen(ta, count):
    lib = ta._lib.lib
    x = edge_u64(count, 2300 + count)
    with Case(ta, f"narrow {count}") as c:
        a, o = c.inp(x, 8, word=8), c.out(4 * count, 4)
        y = c.run(lambda: lib.toyni_narrow_u64_to_u32(a.ptr, o.ptr, count, None))[0]
    same(y, reduce_u64(x), f"narrow {count}")
    with Case(ta, f"widen {count}") as c:
        a, o = c.inp(y, 12), c.out(8 * count, 8, word=8)
        z = c.run(lambda: lib.toyni_widen_u32_to_u64(a.ptr, o.ptr, count, None))[0]
    same(z, y, f"widen {count}")


@pytest.mark.parametrize("nbytes", [64, 64 * 1001])
def test_chacha20_fill(ta, nbytes):
    key = bytes(range(7, 39))
    kb = np.frombuffer(key, dtype=np.uint8).copy()
    nonce = 0x0123456789ABCDEF
    with Case(ta, f"chacha20 {nbytes}") as c:
        o = c.out(nbytes, 0, word=1)
        y = c.run(lambda: ta._lib.lib.toyni_chacha20_fill_device(o.ptr, nbytes, kb.ctypes.data, nonce, None), canonical=False)[0]
    same(y, ref_prover.chacha20_keystream(key, [0, nonce & 0xFFFFFFFF, nonce >> 32], nbytes), f"chacha20 {nbytes}")


def test_fourstep_twiddle_touches_only_its_rows(ta):
    log_n, rows, row_len, row0 = 12, 8, 64, 3
    n = 1 << log_n
    ctx = ctx_of(ta, log_n)
    x = edge_residues((rows + 2) * row_len, 2400)
    w = oracle.root_of_unity(log_n)
    for inverse in (0, 1):
        with Case(ta, f"fourstep inv={inverse}") as c:
            a = c.inout(x, 4)
            y = c.run(lambda: ta._lib.lib.toyni_fourstep_twiddle_device(ctx.handle, a.ptr, rows, row_len, row0, inverse, None))[0]
        ww = pow(w, P - 2, P) if inverse else w
        want = x.astype(np.uint64).copy()
        for r in range(rows):
            for k in range(row_len):
                want[r * row_len + k] = int(x[r * row_len + k]) * pow(ww, ((row0 + r) * k) % n, P) % P
        same(y, want, f"fourstep inv={inverse} (rows past rows * row_len unchanged)")


def test_slab_pass_world4(ta):
    """The slab pass of rank 1 of 4 at a 4-byte offset: forward = M1-point column transforms times w_n^((col_base + c) k1), inverse
    = the inverse column transforms (1/M1); nothing outside the slab touched."""
    log_n, world, rank = 16, 4, 1
    n = 1 << log_n
    ctx = ctx_of(ta, log_n)
    m1 = int(ta._lib.lib.toyni_ntt_ctx_first_pass_points(ctx.handle))
    cols = n // m1 // world
    col_base = rank * cols
    x = edge_residues(m1 * cols, 2500)
    xc = x.reshape(m1, cols).astype(np.uint64)
    w = oracle.root_of_unity(log_n)
    for inverse in (0, 1):
        with Case(ta, f"slab pass inv={inverse}") as c:
            a = c.inout(x, 4)
            y = c.run(lambda: ta._lib.lib.toyni_ntt_slab_pass_device(ctx.handle, a.ptr, cols, col_base, inverse, None))[0].reshape(m1, cols)
        for cc in (0, 1, cols // 2, cols - 1):
            if inverse:
                want = oracle.intt(xc[:, cc])
            else:
                want = oracle.ntt(xc[:, cc])
                want = np.array([int(v) * pow(w, ((col_base + cc) * k1) % n, P) % P for k1, v in enumerate(want)], dtype=np.uint64)
            same(y[:, cc], want, f"slab pass inv={inverse} column {cc}")


@pytest.mark.parametrize("log_n", [16, 22, 24])
def test_slab_relayout_and_rows_world4(ta, log_n):
    """Rank 1 of 4 either side of the exchange, 16-byte aligned buffers: the relayout alone and the relayout fused with the size-S1
    row transforms, forward (received pieces [4][r][w] -> rows [r][S1]) and inverse (rows -> pieces).  Expected values from the
    oracle alone: F = the M1-point column transforms of the input slabs, rows = X[(row0 + i) + M1 k'].  At 2^16 (rows of 256 points)
    the rows step is always the two-step form; at 2^22 and 2^24 it is the fused form wherever the row passes can address the pieces
    (which shape fuses is pinned in tests/test_gpu_multi.py; the form that ran is named in every message here).  The inverse rows form
    may overwrite d_in (include/toyni_hip.h), so its input is checked only for its guards: (d) is waived there."""
    world, h = 4, 1
    n = 1 << log_n
    lib = ta._lib.lib
    big = ctx_of(ta, log_n)
    m1 = int(lib.toyni_ntt_ctx_first_pass_points(big.handle))
    s1 = n // m1
    row = ctx_of(ta, s1.bit_length() - 1)
    r, w = m1 // world, s1 // world
    x = edge_residues(n, 2600 + log_n).astype(np.uint64)
    X = oracle.ntt(x)
    pts = oracle.domain_elements(n, 1)                                  # w_n^e
    k1 = np.arange(h * r, (h + 1) * r, dtype=np.uint64)[:, None]
    F = np.empty((world, r, w), dtype=np.uint64)                       # block h of each slab's column transforms, untwiddled
    recv = np.empty((world, r, w), dtype=np.uint64)                    # ... and twiddled: what rank h receives
    for g in range(world):
        cols = x.reshape(m1, s1)[:, g * w:(g + 1) * w]
        Fg = np.stack([oracle.ntt(cols[:, c]) for c in range(w)], axis=1)[h * r:(h + 1) * r]
        F[g] = Fg
        e = ((np.arange(g * w, (g + 1) * w, dtype=np.uint64)[None, :] * k1) % np.uint64(n)).astype(np.int64)
        recv[g] = Fg * pts[e].astype(np.uint64) % np.uint64(P)        # (< 2^62: no overflow)
    rows = X[(h * r + np.arange(r))[:, None] + m1 * np.arange(s1)[None, :]]
    pre = np.stack([oracle.intt(rows[i]) for i in range(r)])          # the rows before the size-S1 transforms
    recv32, rows32, pre32 = recv.astype(np.uint32), rows.astype(np.uint32), pre.astype(np.uint32)
    fused = ctypes.c_int(-1)
    for inverse, src, want_relayout, want_rows in ((0, recv32, pre, rows), (1, None, F, F)):
        with Case(ta, f"slab relayout 2^{log_n} inv={inverse}") as c:
            a, o = c.inp(pre32 if inverse else src, 0), c.out(4 * r * s1, 0)
            y = c.run(lambda: lib.toyni_ntt_slab_relayout_device(big.handle, a.ptr, o.ptr, r, h * r, world, inverse, None))[0]
        same(y, want_relayout, f"slab relayout 2^{log_n} inv={inverse}")
        with Case(ta, f"slab rows 2^{log_n} inv={inverse}") as c:
            if inverse:
                a = c.inout(rows32, 0)                                # (d) waived: the inverse form may overwrite d_in
            else:
                a = c.inp(src, 0)
            o = c.out(4 * r * s1, 0)
            y = c.run(lambda: lib.toyni_ntt_slab_rows_device(big.handle, row.handle, a.ptr, o.ptr, r, h * r, world, inverse,
                                                             ctypes.byref(fused), None))[0]
        same(y, want_rows, f"slab rows 2^{log_n} inv={inverse} (fused form: {fused.value})")
        if log_n == 16:
            assert fused.value == 0, "rows of 256 points are single-pass transforms: the two-step form"


# ---------------------------------------------------------------- zero-size work and refused arguments
def test_zero_size_work_writes_nothing(ta):
    lib = ta._lib.lib
    ctx = ctx_of(ta, 12)
    beta4 = np.zeros(4, dtype=np.uint32)
    with Case(ta, "zero-size") as c:
        a, o = c.inp(edge_residues(64, 1), 4), c.out(256, 4)
        o8 = c.out(256, 8, word=8)
        lv = c.inp(np.zeros(32 * 127, dtype=np.uint8), 0, word=1)       # 16-byte aligned, as the openings require
        calls = {
            "ntt batch 0": lambda: lib.toyni_ntt_device(ctx.handle, a.ptr, o.ptr, 0, 0, None),
            "coset batch 0": lambda: lib.toyni_coset_ntt_device(ctx.handle, a.ptr, o.ptr, 0, 7, 1, None),
            "ext batch 0": lambda: lib.toyni_ntt_ext_batch_device(ctx.handle, a.ptr, o.ptr, 0, 7, 0, None),
            "lde batch 0": lambda: lib.toyni_lde_device(ctx.handle, a.ptr, o.ptr, 0, 2, 7, None),
            "lde_ext batch 0": lambda: lib.toyni_lde_ext_batch_device(ctx.handle, a.ptr, o.ptr, 0, 2, 7, None),
            "u64 batch 0": lambda: lib.toyni_ntt_device_u64(ctx.handle, o8.ptr, 0, 0, None),
            "domain m 0": lambda: lib.toyni_domain_elements_device(ctx.handle, o.ptr, 0, 7, None),
            "fold m 0": lambda: lib.toyni_fri_fold_device(ctx.handle, a.ptr, o.ptr, 0, 5, 7, None),
            "fold_xs m 0": lambda: lib.toyni_fri_fold_xs_device(a.ptr, a.ptr, o.ptr, 0, 5, None),
            "fold_ext m 0": lambda: lib.toyni_fri_fold_ext_device(ctx.handle, a.ptr, o.ptr, 0, beta4.ctypes.data, 7, None),
            "fold_ext_xs m 0": lambda: lib.toyni_fri_fold_ext_xs_device(a.ptr, a.ptr, o.ptr, 0, beta4.ctypes.data, None),
            "fold layers 0": lambda: lib.toyni_fri_fold_layers_device(ctx.handle, a.ptr, o.ptr, None, 0, 7, None),
            "narrow 0": lambda: lib.toyni_narrow_u64_to_u32(o8.ptr, o.ptr, 0, None),
            "widen 0": lambda: lib.toyni_widen_u32_to_u64(a.ptr, o8.ptr, 0, None),
            "fourstep rows 0": lambda: lib.toyni_fourstep_twiddle_device(ctx.handle, o.ptr, 0, 64, 0, 0, None),
            "open nidx 0": lambda: lib.toyni_merkle_open_device(lv.ptr, 64, a.ptr, None, a.ptr, 0, o8.ptr, None),
        }
        for what, call in calls.items():
            c._prepare("sentinel")
            rc = call()
            assert rc == 0, f"{what}: status {rc}"
            c.mem.sync()
            c.untouched()
            for g in c.outs:
                g.check(what)


def test_refused_arguments_write_nothing(ta):
    """Argument errors are reported before anything is enqueued: the output payload and its guards stay as they were."""
    lib = ta._lib.lib
    ctx = ctx_of(ta, 12)
    ctx16 = ctx_of(ta, 16)
    row = ctx_of(ta, 16 - (int(lib.toyni_ntt_ctx_first_pass_points(ctx16.handle)).bit_length() - 1))
    beta_bad = np.array([1, 2, P, 3], dtype=np.uint32)
    beta_ok = np.array([1, 2, 3, 4], dtype=np.uint32)
    with Case(ta, "refused") as c:
        a = c.inp(edge_residues(1 << 16, 2), 0)
        a4 = c.inp(edge_residues(1 << 16, 3), 4)
        o, o4 = c.out(4 << 16, 0, guard=1 << 18), c.out(4 << 16, 4, guard=1 << 18)
        key = np.zeros(32, dtype=np.uint8)
        u8 = c.out(512, 8, word=8)
        calls = {
            "u64 transform misaligned": (lambda: lib.toyni_ntt_device_u64(ctx.handle, o4.ptr, 1, 0, None), E_RANGE),
            "narrow misaligned u64 in": (lambda: lib.toyni_narrow_u64_to_u32(a4.ptr, o.ptr, 16, None), E_RANGE),
            "narrow misaligned u32 out": (lambda: lib.toyni_narrow_u64_to_u32(u8.ptr, o.ptr + 2, 16, None), E_RANGE),
            "widen misaligned u64 out": (lambda: lib.toyni_widen_u32_to_u64(a.ptr, o4.ptr, 16, None), E_RANGE),
            "widen misaligned u32 in": (lambda: lib.toyni_widen_u32_to_u64(a.ptr + 2, u8.ptr, 16, None), E_RANGE),
            "fold beta = p": (lambda: lib.toyni_fri_fold_device(ctx.handle, a.ptr, o.ptr, 64, P, 7, None), E_RANGE),
            "fold odd m": (lambda: lib.toyni_fri_fold_device(ctx.handle, a.ptr, o.ptr, 63, 5, 7, None), E_ODD),
            "fold x0 = 0": (lambda: lib.toyni_fri_fold_device(ctx.handle, a.ptr, o.ptr, 64, 5, 0, None), E_ZERO_INV),
            "fold_xs beta = p": (lambda: lib.toyni_fri_fold_xs_device(a.ptr, a.ptr, o.ptr, 64, P, None), E_RANGE),
            "fold_xs odd m": (lambda: lib.toyni_fri_fold_xs_device(a.ptr, a.ptr, o.ptr, 7, 5, None), E_ODD),
            "fold_ext beta >= p": (lambda: lib.toyni_fri_fold_ext_device(ctx.handle, a.ptr, o.ptr, 64, beta_bad.ctypes.data, 7, None), E_RANGE),
            "fold_ext misaligned evals": (lambda: lib.toyni_fri_fold_ext_device(ctx.handle, a4.ptr, o.ptr, 64, beta_ok.ctypes.data, 7, None), E_RANGE),
            "fold_ext misaligned out": (lambda: lib.toyni_fri_fold_ext_device(ctx.handle, a.ptr, o4.ptr, 64, beta_ok.ctypes.data, 7, None), E_RANGE),
            "fold_ext_xs misaligned": (lambda: lib.toyni_fri_fold_ext_xs_device(a4.ptr, a.ptr, o.ptr, 64, beta_ok.ctypes.data, None), E_RANGE),
            "fold_ext_xs misaligned out": (lambda: lib.toyni_fri_fold_ext_xs_device(a.ptr, a.ptr, o4.ptr, 64, beta_ok.ctypes.data, None), E_RANGE),
            "fold_ext_xs odd m": (lambda: lib.toyni_fri_fold_ext_xs_device(a.ptr, a.ptr, o.ptr, 9, beta_ok.ctypes.data, None), E_ODD),
            "fold layers shift 0": (lambda: lib.toyni_fri_fold_layers_device(ctx.handle, a.ptr, o.ptr, beta_ok.ctypes.data, 2, 0, None), E_ZERO_INV),
            "coset shift p": (lambda: lib.toyni_coset_ntt_device(ctx.handle, a.ptr, o.ptr, 1, P, 0, None), E_RANGE),
            "lde in place": (lambda: lib.toyni_lde_device(ctx.handle, o.ptr, o.ptr, 1, 2, 7, None), E_RANGE),
            "merkle misaligned levels": (lambda: lib.toyni_merkle_commit_device(a.ptr, None, 64, o4.ptr, None), E_RANGE),
            "merkle misaligned salts": (lambda: lib.toyni_merkle_commit_device(a.ptr, a4.ptr, 64, o.ptr, None), E_RANGE),
            "open misaligned out": (lambda: lib.toyni_merkle_open_device(a.ptr, 64, a.ptr, None, a.ptr, 1, o4.ptr, None), E_RANGE),
            "chacha misaligned": (lambda: lib.toyni_chacha20_fill_device(o4.ptr, 64, key.ctypes.data, 0, None), E_RANGE),
            "chacha ragged": (lambda: lib.toyni_chacha20_fill_device(o.ptr, 100, key.ctypes.data, 0, None), E_RANGE),
            "relayout misaligned": (lambda: lib.toyni_ntt_slab_relayout_device(ctx16.handle, a4.ptr, o.ptr, 4, 0, 4, 0, None), E_RANGE),
            "slab rows misaligned": (lambda: lib.toyni_ntt_slab_rows_device(ctx16.handle, row.handle, a.ptr, o4.ptr, 4, 0, 4, 0, None, None), E_RANGE),
        }
        for what, (call, want) in calls.items():
            c._prepare("sentinel")
            rc = call()
            assert rc == want, f"{what}: status {rc}, expected {want}"
            c.mem.sync()
            c.untouched()
            for g in c.outs:
                g.check(what)
