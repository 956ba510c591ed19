"""The instruction set of constraint programs (include/toyni_hip.h 3f) as a vectorised numpy model, plus generators of programs, the
model of the multi-column DEEP combination (3e) and the launcher's sizing rule restated.  Shared by the tests of the AIR quotient, the
DEEP combination and the two-column proof; imports nothing from the library."""
import numpy as np

P = 2013265921
GEN_2_27 = 440564289
CELL, CONST, X, XINV, ADD, SUB, MUL, EMIT = range(8)


def powmod_vec(a, e):
    r = np.ones_like(a, dtype=np.uint64)
    a = a.astype(np.uint64)
    while e:
        if e & 1:
            r = r * a % np.uint64(P)
        a = a * a % np.uint64(P)
        e >>= 1
    return r


def coset_points(n, shift):
    w = pow(GEN_2_27, (1 << 27) // n, P)
    xs = np.array([shift], dtype=np.uint64)
    while xs.size < n:
        xs = np.concatenate([xs, xs * np.uint64(pow(w, xs.size, P)) % np.uint64(P)])
    return xs


def deep_model(m, terms, blowup, shift, z):
    """m: (width, N) uint64 canonical; terms: (column, rotation, alpha, value).  x_i = z gives 0 (Fermat: 0^(p-2) = 0)."""
    n = m.shape[1]
    num = np.zeros(n, dtype=np.uint64)
    for c, rot, a, v in terms:
        col = np.roll(m[c], -(rot * blowup) % n)
        num = (num + (col + np.uint64(P - v)) % np.uint64(P) * np.uint64(a)) % np.uint64(P)
    den = (coset_points(n, shift) + np.uint64(P - z)) % np.uint64(P)
    return (num * powmod_vec(den, P - 2) % np.uint64(P)).astype(np.uint32)


def air_launch_shape(nregs, divides, log_b):
    """air_launch_shape (toyni_amd/csrc/prover_kernels.hpp) restated: (threads, dynamic LDS bytes, the 1 / Z_H class table is in LDS)."""
    threads = next(t for t in (256, 128, 64) if nregs * t * 16 <= 65536 or t == 64)
    zh = int(bool(divides) and log_b <= 8 and nregs * threads * 16 + (4 << log_b) <= 65536)
    return threads, nregs * threads * 16 + zh * (4 << log_b), zh


def air_model(insns, mats, n_points, log_blowup, shift, weights):
    """insns: (op, dst, a, b, imm) tuples; mats: list of (width, N) arrays of canonical residues.  Returns (c, q) as uint32 arrays.
    Inverses are Fermat powers, so the inverse of 0 is 0."""
    p = np.uint64(P)
    N, B = n_points, 1 << log_blowup
    xs = coset_points(N, shift)
    regs = {}
    c = np.zeros(N, dtype=np.uint64)
    undivided = np.zeros(N, dtype=np.uint64)
    divides = False
    for op, dst, a, b, imm in insns:
        if op == CELL:
            regs[dst] = np.roll(np.asarray(mats[b][imm], dtype=np.uint64), -((a * B) % N))
        elif op == CONST:
            regs[dst] = np.full(N, imm, dtype=np.uint64)
        elif op == X:
            regs[dst] = xs.copy()
        elif op == XINV:
            regs[dst] = powmod_vec((xs + np.uint64(P - imm)) % p, P - 2)
        elif op == ADD:
            regs[dst] = (regs[a] + regs[b]) % p
        elif op == SUB:
            regs[dst] = (regs[a] + (p - regs[b])) % p
        elif op == MUL:
            regs[dst] = regs[a] * regs[b] % p
        elif op == EMIT:
            term = regs[a] * np.uint64(weights[imm]) % p
            if b:
                undivided = (undivided + term) % p
            else:
                c, divides = (c + term) % p, True
        else:
            raise ValueError(op)
    q = undivided
    if divides:
        zh = (powmod_vec(xs, N >> log_blowup) + np.uint64(P - 1)) % p
        q = (c * powmod_vec(zh, P - 2) + undivided) % p
    return c.astype(np.uint32), q.astype(np.uint32)


def fib_program(n_rows):
    """The quotient of toyni_fib_quotient_device (src/fibonacci.rs:133-150) as the 13 instructions of the header; weights = [1]."""
    g = pow(GEN_2_27, (1 << 27) // n_rows, P)
    return [(CELL, 0, 0, 0, 0), (CELL, 1, 1 % n_rows, 0, 0), (CELL, 2, 2 % n_rows, 0, 0), (ADD, 0, 1, 0, 0), (SUB, 0, 2, 0, 0), (X, 1, 0, 0, 0),
            (CONST, 2, 0, 0, pow(g, n_rows - 1, P)), (SUB, 2, 1, 2, 0), (MUL, 0, 0, 2, 0), (CONST, 2, 0, 0, pow(g, n_rows - 2, P)), (SUB, 2, 1, 2, 0),
            (MUL, 0, 0, 2, 0), (EMIT, 0, 0, 0, 0)]


def random_program(rng, nregs, length, widths, rows, nconstraints, xinv_point, may_divide=True):
    """A valid program of exactly max(length, nregs + nconstraints + 1) instructions: the first nregs write every register once (a CELL,
    a CONST, an X and an XINV lead), the rest combine any two; the last nconstraints + 1 emit every number (number 0 twice, divided and
    undivided alternately).  Rotations reach rows - 1 (capped at 255), so reads wrap past N."""
    insns = []
    nemit = nconstraints + 1
    k = 0
    while len(insns) + nemit < length or k < nregs:
        dst = k if k < nregs else int(rng.integers(0, nregs))
        written = min(k, nregs)
        kind = k if k < 4 else int(rng.integers(0, 12))
        if kind == 0 or written == 0:
            m = int(rng.integers(0, len(widths)))
            rot = min(rows - 1, 255) if k % 3 == 2 else int(rng.integers(0, min(rows, 256)))
            insns.append((CELL, dst, rot, m, int(rng.integers(0, widths[m]))))
        elif kind == 1:
            insns.append((CONST, dst, 0, 0, [0, 1, P - 1, int(rng.integers(0, P))][k % 4]))
        elif kind == 2:
            insns.append((X, dst, 0, 0, 0))
        elif kind == 3:
            insns.append((XINV, dst, 0, 0, xinv_point))
        else:
            insns.append((ADD + kind % 3, dst, int(rng.integers(0, written)), int(rng.integers(0, written)), 0))
        k += 1
    for e in range(nemit):
        insns.append((EMIT, 0, int(rng.integers(0, nregs)), (e & 1) if may_divide else 1, e % nconstraints))
    return insns
