"""Guard-banded buffers and field-edge inputs for the GPU tests (a plain module, imported like tests/dispatch_matrix.py).

Guarded(mem, payload_bytes, offset, guard) allocates ONE block laid out as

    [front guard][offset bytes][payload][back guard]

and fills all of it with the sentinel byte 0xA5 (0xA5A5A5A5 >= p, so no canonical u32 or u64 output can equal it).  Each guard is at
least 64 KiB, so that an overrun by a whole tile still lands inside the allocation, where check() sees it instead of slack that
hipMalloc rounded up and nothing reads.  offset in {0, 4, 8, 12} hands the kernel a pointer that is 4-byte but not 16-byte aligned
(the block itself is 256-byte aligned and the guard a multiple of 16).  `offset` bytes belong to the front guard for check().

`mem` is the library module (toyni_amd: toyni_malloc / toyni_memcpy_*), or HostMem(): host memory behind the same five calls, which
the CPU tests use as a stand-in and the host-slice entry points use as guarded numpy arrays.

refill("random") refills the guards with seeded random canonical words: a case run once with sentinel guards and once with random
ones around its inputs must give identical outputs, or the kernel read something outside its inputs."""
import ctypes

import numpy as np

P = 2013265921
SENTINEL = 0xA5
GUARD_MIN = 64 << 10
CHECK_CHUNK = 64 << 20                 # bytes of a guard compared per download
R_MONT = (1 << 32) % P                 # the Montgomery radix 2^32 mod p
R_INV = pow(R_MONT, -1, P)


class HostMem:
    """Host memory behind the calls Guarded makes of the library (CPU stand-in, and guards around host-slice arguments)."""

    def __init__(self):
        self._blocks = {}

    def malloc(self, nbytes):
        a = np.empty(nbytes + 256, dtype=np.uint8)
        ptr = (a.ctypes.data + 255) & ~255          # the alignment hipMalloc gives
        self._blocks[ptr] = a
        return ptr

    def free(self, ptr):
        del self._blocks[ptr]

    def h2d(self, dst, src, nbytes):
        ctypes.memmove(dst, src, nbytes)

    def d2h(self, dst, src, nbytes):
        ctypes.memmove(dst, src, nbytes)

    def memset(self, ptr, value, nbytes):
        ctypes.memset(ptr, value, nbytes)

    def sync(self):
        pass

    def view(self, ptr, nbytes, dtype=np.uint8):
        """A numpy view of nbytes at ptr (host-slice entry points take it as their argument)."""
        return np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(ptr)).view(dtype)


class DevMem:
    """Device memory through the library's plumbing calls (include/toyni_hip.h section 4)."""

    def __init__(self, ta):
        self.ta = ta
        self.lib = ta._lib.lib

    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        self.ta._lib.check(self.lib.toyni_malloc(ctypes.byref(p), nbytes), "malloc")
        return p.value

    def free(self, ptr):
        self.lib.toyni_free(ptr)

    def h2d(self, dst, src, nbytes):
        assert self.lib.toyni_memcpy_h2d(dst, src, nbytes) == 0

    def d2h(self, dst, src, nbytes):
        assert self.lib.toyni_memcpy_d2h(dst, src, nbytes) == 0

    def memset(self, ptr, value, nbytes):
        assert self.lib.toyni_memset_async(ptr, value, nbytes, None) == 0
        self.sync()

    def sync(self):
        assert self.lib.toyni_stream_synchronize(None, None) == 0


def memory_of(mem):
    if isinstance(mem, (HostMem, DevMem)):
        return mem
    return DevMem(mem)                    # the toyni_amd module


def guard_pattern(kind, nbytes, seed, word=4):
    """Guard contents: 0xA5 bytes, or seeded random canonical words (u32, or u64 for word=8)."""
    if kind == "sentinel":
        return np.full(nbytes, SENTINEL, dtype=np.uint8)
    assert kind == "random", kind
    rng = np.random.default_rng(seed)
    words = rng.integers(0, P, size=(nbytes + word - 1) // word, dtype=np.uint64)
    return words.astype(np.uint32 if word == 4 else np.uint64).view(np.uint8)[:nbytes].copy()


class Guarded:
    """One guard-banded buffer; ptr is the payload.  word = 4 (packed u32), 8 (u64) or 1 (bytes: Merkle levels, opening records)."""

    def __init__(self, mem, payload_bytes, offset=0, guard=GUARD_MIN, word=4, seed=0):
        """guard: bytes of each guard, raised to GUARD_MIN; callers pass at least one transform or layer of their case."""
        assert offset in (0, 4, 8, 12) or offset % 16 == 0, offset
        self.mem = memory_of(mem)
        self.nbytes = int(payload_bytes)
        self.offset = offset
        self.guard = (max(int(guard), GUARD_MIN) + 15) & ~15
        self.word = word
        self.seed = seed
        self.front = self.guard + offset
        self.total = self.front + self.nbytes + self.guard
        self.base = self.mem.malloc(self.total)
        self.ptr = self.base + self.front
        self._guards = None
        self.fill_sentinel()

    # ---- contents
    def fill_sentinel(self):
        """The whole block (guards AND payload) to 0xA5: an output word the call does not write stays >= p."""
        self.mem.memset(self.base, SENTINEL, self.total)
        self._guards = ("sentinel", None, None)

    def refill(self, pattern):
        """Refill both guards (not the payload) with `pattern` ("sentinel" or "random")."""
        front = guard_pattern(pattern, self.front, self.seed * 2 + 1, max(self.word, 4))
        back = guard_pattern(pattern, self.guard, self.seed * 2 + 2, max(self.word, 4))
        self.mem.h2d(self.base, front.ctypes.data, front.nbytes)
        self.mem.h2d(self.ptr + self.nbytes, back.ctypes.data, back.nbytes)
        self._guards = (pattern, None, None) if pattern == "sentinel" else (pattern, front, back)

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes, "upload past the payload"
        if arr.nbytes:
            self.mem.h2d(self.ptr + offset, arr.ctypes.data, arr.nbytes)

    def download(self, dtype=None, count=None, offset=0):
        dtype = np.dtype(dtype or {1: np.uint8, 4: np.uint32, 8: np.uint64}[self.word])
        if count is None:
            count = (self.nbytes - offset) // dtype.itemsize
        out = np.empty(count, dtype=dtype)
        assert offset + out.nbytes <= self.nbytes, "download past the payload"
        if out.nbytes:
            self.mem.d2h(out.ctypes.data, self.ptr + offset, out.nbytes)
        return out

    # ---- checks
    def _damage(self, ptr, nbytes, want):
        """(first, last) damaged byte offsets of the region at ptr, or None.  Sentinel regions (want None) are read in chunks, so a
        guard of a whole large transform costs no host array of its size."""
        first = last = None
        for off in range(0, nbytes, CHECK_CHUNK):
            k = min(CHECK_CHUNK, nbytes - off)
            got = np.empty(k, dtype=np.uint8)
            self.mem.d2h(got.ctypes.data, ptr + off, k)
            bad = np.flatnonzero(got != (SENTINEL if want is None else want[off:off + k]))
            if bad.size:
                first = off + int(bad[0]) if first is None else first
                last = off + int(bad[-1])
        return None if first is None else (first, last)

    def check(self, what="buffer"):
        """Both guards as they were filled; raises AssertionError naming the first damaged byte and the length of the damage."""
        _, front_want, back_want = self._guards
        d = self._damage(self.base, self.front, front_want)
        if d:
            first, last = d
            raise AssertionError(f"{what}: front guard damaged {self.front - first} bytes before the payload start "
                                 f"({(self.front - first + 3) // 4} words), {last - first + 1} bytes long")
        d = self._damage(self.ptr + self.nbytes, self.guard, back_want)
        if d:
            first, last = d
            raise AssertionError(f"{what}: back guard damaged {first} bytes past the payload end "
                                 f"(word {first // 4} past it), {last - first + 1} bytes long")

    def free(self, check=True):
        if self.base is None:
            return
        try:
            if check:
                self.check()
        finally:
            self.mem.free(self.base)
            self.base = None


# ---------------------------------------------------------------- field-edge inputs
def edge_classes():
    """Every edge value the lazy reductions care about: named so that a test can say which one it is missing."""
    half = (P - 1) // 2
    return {
        "zero": 0, "one": 1, "two": 2, "p-1": P - 1, "p-2": P - 2,
        "(p-1)/2": half, "(p+1)/2": half + 1,
        "2^27": 1 << 27, "2^27-1": (1 << 27) - 1, "2^27+1": (1 << 27) + 1, "2^30": 1 << 30,
        # Montgomery form v * 2^32 mod p = 0 / 1 / p-1, and inverse form v * 2^-32 mod p = 1 / p-1
        "mont=1": R_INV, "mont=p-1": P - R_INV,
        "invmont=1": R_MONT, "invmont=p-1": P - R_MONT,
    }


def edge_residues(n, seed, frac=0.25):
    """n canonical residues (uint32): seeded random ones, a fraction `frac` of them replaced by edge values, every edge class at the
    front, and from n/2 on a run of p-1 and alternating 0 / p-1 blocks of 1, 2, 4 ... words, so that butterflies pair edges with
    edges at every distance."""
    rng = np.random.default_rng(seed)
    pool = np.array(sorted(set(edge_classes().values())), dtype=np.uint64)
    out = rng.integers(0, P, size=n, dtype=np.uint64)
    pick = rng.random(n) < frac
    out[pick] = rng.choice(pool, size=int(pick.sum()))
    k = min(n, pool.size)
    out[:k] = pool[:k]
    if n >= 4:
        h = n // 2
        kh = min(h, pool.size)
        out[h:h + kh] = pool[::-1][:kh]          # the partners at distance n/2 of the front classes are edges too
        start = h + kh
        run = min(max(h // 4, 1), 256)
        out[start:start + run] = P - 1
        pos, blk, val = start + run, 1, 0
        while pos < n and blk <= max(1, h // 8):
            for _ in range(2):
                out[pos:pos + blk] = val
                val = P - 1 - val
                pos += blk
            blk *= 2
    return out.astype(np.uint32)


U64_NONCANONICAL = (P, 2 * P, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1)


def edge_u64(n, seed, frac=0.25):
    """n uint64 inputs for the u64 entry points: edge_residues plus the non-canonical values those entry points reduce (like
    BabyBear::new: a full v % p), every one of them present and more scattered at random."""
    rng = np.random.default_rng(seed ^ 0x55AA)
    out = edge_residues(n, seed, frac).astype(np.uint64)
    nc = np.array(U64_NONCANONICAL, dtype=np.uint64)
    k = min(n, nc.size)
    if n > nc.size + len(edge_classes()):
        out[-k:] = nc[:k]
        pick = rng.random(n) < frac / 4
        out[pick] = rng.choice(nc, size=int(pick.sum()))
    else:
        out[:k] = nc[:k]
    return out


def reduce_u64(x):
    """What the u64 entry points do with an input: v % p."""
    return (np.asarray(x, dtype=np.uint64) % np.uint64(P)).astype(np.uint64)
