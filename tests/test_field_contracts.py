"""The operand domains of the lazy field arithmetic (toyni_amd/csrc/bb_field.hpp), checked in every kernel body the CPU can run.

Most primitives of bb_field.hpp are correct only on a restricted domain stated in their comments (canonical operands for bb_add,
x < 2p for bb_reduce_2p, at most four products of canonical factors for mont_reduce_wide, ...), and a kernel that leaves such a
domain still returns the right words until a 64-bit sum actually wraps: on one input in millions.  Each primitive therefore calls
TOYNI_FIELD_CONTRACT at its top -- empty in every product build and in all device code -- and the CONTRACT builds here pull in
tests/emu/field_contracts.hpp with -include, which evaluates every domain exactly (sums in unsigned __int128), counts calls and
violations per primitive, keeps the first violation with its operands and the driver's case tag, and prints one CONTRACT line per
primitive at exit.

Twelve programs run under the contracts: the nine of tests/emu with exactly the arguments their own tests pass, the two drivers of
tests/sim (plain runs, no mutation pass), and tests/sim/sim_pointwise.cpp -- the nine barrier-free __global__ functions whose
arithmetic text is in toyni_hip.hip and that no other CPU program runs, each compared with the oracle or with the defining sum in
host integers.  Per program: it ends as its plain test expects, no line reports a violation, and REACH names the primitives it must
have called (a contract nobody reaches proves nothing).  The emu programs run a second time on SATURATED operands (every data word
p - 1, every constant 1069547521, whose Montgomery form is p - 1: each product is (p - 1)^2, the bound the comments claim), their
outputs checked here in Python integers or by the oracle.  --contract-selftest gives the harness teeth: toys that break each
contract exactly once must be reported under their own primitive and tag.

Not run under the contracts: the three-pass cases 2^23 .. 2^26 of tests/test_emu.py (ten minutes of CPU time on top of the
list above, which steps three-pass plans at 2^21 and 2^22) and the sanitized builds (cases the plain runs have as well).

CPU only, stand-alone programs, no sanitizer; the binaries are built here into the existing build/ folders with a _contracts suffix."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache

import numpy as np

import __graft_entry__ as entry
import ext_model as em
import oracle
import rows_common as rc
import test_emu
import test_emu_rows
import test_emu_scan_ext
import test_sim_scan_ext
import test_sim_schedules
from air_model import air_model, deep_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
SIM = os.path.join(ROOT, "tests", "sim")
HEADER = os.path.join(EMU, "field_contracts.hpp")
ORACLE_C = os.path.join(ROOT, "oracle", "toyni_oracle.c")
P = 2013265921
SAT_X = 1069547521                       # the plain value whose Montgomery form is p - 1 (tests/guarded.py: mont=p-1)
assert SAT_X * (1 << 32) % P == P - 1

PRIMITIVES = ["bb_add", "bb_sub", "bb_sub_lazy", "bb_reduce_2p", "bb_halve", "mont_mul_lazy", "mont_mul", "mont_dot_sub", "mont_dot2",
              "mont_reduce_wide", "wide_acc"]
WORKERS = 8

# program -> (needs the oracle object, arguments of its plain test, how the plain test knows it ended well)
EMU_PROGRAMS = {
    "emu_ntt": (True, test_emu.EMU_NTT_ARGS, "ALL OK"),
    "emu_seed_hoist": (True, [], "ALL OK"),
    "emu_deep": (False, [], "DONE"),
    "emu_deep_ext": (False, [], "DONE"),
    "emu_air": (False, [], "DONE"),
    "emu_rows": (False, [str(test_emu_rows.MAX_WIDTH)], "DONE"),
    "emu_scan": (False, [], "DONE"),
    "emu_scan_ext": (False, [], "DONE"),
    "emu_fold_ext_commit": (False, [], "DONE"),
}
# the saturated run of the programs that have one (gated by an argument: the plain tests' outputs are what they were).  emu_ntt: every
# word p - 1 and alternating 0 / p - 1 through a transform, a coset transform by SAT_X and an LDE, at one size per pass family it
# steps -- the register kernels (2^8), one and two waves per transform (R1: 2^11, 2^12), the single-sweep kernel (2^13, 2^14), the
# two-step and three-step two-pass plans (2^16, 2^18, 2^20; p-1: two-step alone), the 64-wide shapes (w0), three passes (2^21) and
# the 2048-point latency plan (Q1) -- and the Ext fold with beta = (SAT_X, SAT_X, SAT_X, SAT_X)
SATURATED = {
    "emu_ntt": ["0", "S8", "R1", "S11", "S12", "R0", "S13", "S14", "S16", "S18", "S20", "S21", "p-1", "S16", "S20", "w0", "S13", "S16", "w10", "p6",
                "Q1", "S21", "Q0"],
    "emu_deep": ["saturated"],
    "emu_deep_ext": ["saturated"],
    "emu_air": ["saturated"],
    "emu_scan_ext": ["saturated"],
    "emu_fold_ext_commit": ["saturated"],
}

# Which primitives each program must have called.  Filled from what the programs print, then read against the source: it records what
# SHOULD be reached.
#   emu_ntt          butterflies are mont_dot_sub / mont_dot2 with bb_add / bb_sub; the running twiddles mont_mul_lazy; the folds
#                    bb_halve + bb_sub_lazy; the Ext fold mont_dot2.  Its prover steps use the fib kernels, not the term loops.
#   emu_seed_hoist   the two-step column passes alone: dot products, the lazy seeds, no fold
#   emu_deep(_ext)   the four-product groups: wide_acc + mont_reduce_wide; the point inverses mont_mul / bb_sub; Ext adds mont_dot2
#   emu_air          the interpreter: ADD / SUB / MUL and the Z_H inverses
#   emu_rows         SHA-256 leaves of canonical words: no field arithmetic at all (the table says so instead of omitting it)
#   emu_scan         base-field scans: products (mont_mul), sums and shifts (bb_add), the batched inverses
#   emu_scan_ext     Ext products (mont_dot2) and the tower inverse
#   emu_fold_ext_commit  fold_ext_one: bb_halve, bb_sub_lazy, mont_mul, mont_dot2
#   sim_kernels      every transform kernel, the base scans, poly_eval, the quotients
#   sim_scan_ext     as emu_scan_ext
#   sim_pointwise    relayout_quad's lazy chain (mont_mul_lazy), the DEEP term loops (wide_acc, mont_reduce_wide), the Ext fold
REACH = {
    "emu_ntt": {"bb_add", "bb_sub", "bb_sub_lazy", "bb_reduce_2p", "bb_halve", "mont_mul_lazy", "mont_mul", "mont_dot_sub", "mont_dot2"},
    "emu_seed_hoist": {"bb_add", "bb_sub", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot_sub"},
    "emu_deep": {"bb_add", "bb_sub", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_reduce_wide", "wide_acc"},
    "emu_deep_ext": {"bb_add", "bb_sub", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot2", "mont_reduce_wide", "wide_acc"},
    "emu_air": {"bb_add", "bb_sub", "bb_reduce_2p", "mont_mul_lazy", "mont_mul"},
    "emu_rows": set(),
    "emu_scan": {"bb_add", "bb_reduce_2p", "mont_mul_lazy", "mont_mul"},
    "emu_scan_ext": {"bb_add", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot2"},
    "emu_fold_ext_commit": {"bb_add", "bb_sub_lazy", "bb_reduce_2p", "bb_halve", "mont_mul_lazy", "mont_mul", "mont_dot2"},
    "sim_kernels": {"bb_add", "bb_sub", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot_sub", "mont_dot2"},
    "sim_scan_ext": {"bb_add", "bb_reduce_2p", "mont_mul_lazy", "mont_mul", "mont_dot2"},
    "sim_pointwise": {"bb_add", "bb_sub", "bb_sub_lazy", "bb_reduce_2p", "bb_halve", "mont_mul_lazy", "mont_mul", "mont_dot2", "mont_reduce_wide",
                      "wide_acc"},
}
POINTWISE_KERNELS = ["fourstep_twiddle_kernel", "slab_relayout_kernel", "domain_elements_kernel", "deep_combine_kernel", "deep_combine_inline_kernel",
                     "deep_combine_ext_kernel", "deep_combine_ext_inline_kernel", "fri_fold_ext_kernel", "fri_fold_ext_stream_kernel"]
POINTWISE_INSTANTIATIONS = [
    r"fourstep_twiddle_kernel<forward>", r"fourstep_twiddle_kernel<inverse>",
    r"slab_relayout_kernel<forward,four-in-flight\+tail>", r"slab_relayout_kernel<forward,tail-only>",
    r"slab_relayout_kernel<inverse,four-in-flight\+tail>", r"slab_relayout_kernel<inverse,tail-only>",
    r"fri_fold_ext_stream_kernel<.*chunks>grid>", r"fri_fold_ext_stream_kernel<.*ragged-chunk>",
] + [k + "<nterms=%d," % t for k in ("deep_combine_kernel", "deep_combine_ext_kernel") for t in (3, 4, 5, 64, 65)] + \
    [k + "<nterms=%d," % t for k in ("deep_combine_inline_kernel", "deep_combine_ext_inline_kernel") for t in (3, 4, 5, 64)]


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def _oracle_object(build_dir):
    obj = os.path.join(build_dir, "oracle_contracts.o")
    if _stale(obj, [ORACLE_C]):
        os.makedirs(build_dir, exist_ok=True)
        subprocess.check_call(["gcc", "-O2", "-c", "-o", obj, ORACLE_C])
    return obj


@lru_cache(maxsize=None)
def build_contracts(program):
    """The program's source with the contract header in front: g++ -O2 for tests/emu, the ROCm clang++ for tests/sim (as the plain builds)."""
    sim = program.startswith("sim_")
    folder = SIM if sim else EMU
    src, out = os.path.join(folder, program + ".cpp"), os.path.join(folder, "build", program + "_contracts")
    deps = [src, HEADER, os.path.join(EMU, "contract_case.hpp"), ORACLE_C, os.path.join(SIM, "hip_sim.hpp"), os.path.join(ROOT, "include", "toyni_hip.h")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip"))]
    if _stale(out, deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        if sim:   # hip_sim.hpp first: it defines the host forms of the synchronisation macros, which bb_field.hpp keeps when it finds them
            cmd = [entry._host_clang(), "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-unused-const-variable", "-I", CSRC,
                   "-I", os.path.join(ROOT, "include"), "-include", os.path.join(SIM, "hip_sim.hpp"), "-include", HEADER, "-o", out, src]
            if program != "sim_scan_ext":
                cmd.append(_oracle_object(os.path.dirname(out)))
        else:
            cmd = ["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-include", HEADER, "-o", out, src]
            if EMU_PROGRAMS[program][0]:
                cmd.append(_oracle_object(os.path.dirname(out)))
        subprocess.check_call(cmd)
    return out


def _run(program, args, timeout=1800):
    res = subprocess.run([build_contracts(program), *args], capture_output=True, text=True, timeout=timeout)
    return res.returncode, res.stdout, res.stderr


def contract_lines(text):
    """-> {primitive: (calls, violations, what follows)} from the CONTRACT lines of one run."""
    found = {}
    for m in re.finditer(r"^CONTRACT (\w+) calls=(\d+) violations=(\d+)(.*)$", text, re.M):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)), m.group(4).strip())
    return found


def _sum_contracts(runs):
    total = {p: [0, 0, ""] for p in PRIMITIVES}
    for text in runs:
        lines = contract_lines(text)
        assert sorted(lines) == sorted(PRIMITIVES), "one CONTRACT line per primitive:\n" + text[-2000:]
        for p, (calls, violations, rest) in lines.items():
            total[p][0] += calls
            total[p][1] += violations
            total[p][2] = total[p][2] or rest
    return total


def _judge(program, runs):
    """No violation on any line, and every primitive of the reach table called."""
    total = _sum_contracts(runs)
    bad = ["%s: %d violations in %d calls, %s" % (p, v, c, rest) for p, (c, v, rest) in total.items() if v]
    assert not bad, program + " left an operand domain:\n" + "\n".join(bad)
    reached = {p for p, (c, _, _) in total.items() if c}
    assert REACH[program] <= reached, "%s never called %s" % (program, sorted(REACH[program] - reached))
    return total


def _emu_ntt_chunks(args, nchunks=6):
    """emu_ntt's one argument list as several processes (four minutes in one): cut anywhere, every later piece starts with `0` (no
    default size loop a second time) and with the switches in effect at the cut -- pN, wN, QN, RN and bN hold from where they stand
    to the end of the list -- so every case runs exactly once and under the knobs it runs under in the plain test."""
    switch = re.compile(r"^[pwQRb]-?\d+$")
    step = -(-len(args) // nchunks)
    chunks = [list(args[:step])]
    for c in range(step, len(args), step):
        chunks.append(["0"] + [a for a in args[:c] if switch.match(a)] + list(args[c:c + step]))
    return chunks


@lru_cache(maxsize=None)
def _emu_runs():
    """Every emu program on its plain test's arguments and, where it has one, on its saturated cases: the slowest first."""
    jobs = [(p, tuple(EMU_PROGRAMS[p][1])) for p in EMU_PROGRAMS if p != "emu_ntt"] + [(p, tuple(a)) for p, a in SATURATED.items()] + \
           [("emu_ntt", tuple(c)) for c in _emu_ntt_chunks(test_emu.EMU_NTT_ARGS)]
    jobs.sort(key=lambda j: (j[0] != "emu_ntt", j[0] != "emu_seed_hoist"))
    for p in EMU_PROGRAMS:
        build_contracts(p)
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        return dict(zip(jobs, ex.map(lambda j: _run(*j), jobs)))


def _plain(program):
    """-> [(return code, stdout, stderr)] of the program's plain arguments (emu_ntt: one per chunk)."""
    if program == "emu_ntt":
        return [_emu_runs()[("emu_ntt", tuple(c))] for c in _emu_ntt_chunks(test_emu.EMU_NTT_ARGS)]
    return [_emu_runs()[(program, tuple(EMU_PROGRAMS[program][1]))]]


def _saturated(program):
    rc_, out, err = _emu_runs()[(program, tuple(SATURATED[program]))]
    assert rc_ == 0, out[-2000:] + err[-3000:]
    return out, err


def test_every_emu_program_keeps_every_operand_domain():
    chunks = _emu_ntt_chunks(test_emu.EMU_NTT_ARGS)
    cases = [a for c in chunks for a in c if not re.match(r"^[pwQRb]-?\d+$", a) and a != "0"]
    assert cases == [a for a in test_emu.EMU_NTT_ARGS if not re.match(r"^[pwQRb]-?\d+$", a)], "the chunks run the list's cases, each once, in order"
    for program, (_, _, marker) in EMU_PROGRAMS.items():
        for rc_, out, err in _plain(program):
            assert rc_ == 0, program + ":\n" + out[-2000:] + err[-3000:]
            if marker == "ALL OK":
                assert "ALL OK" in out, program + out[-2000:]
            else:
                assert out.split("\n")[-2] == "DONE" and not re.search(r"^BAD [1-9]", out, re.M), program + out[-500:]
            assert "CONTRACT" not in out, "the contract lines belong on stderr: stdout is what the plain build prints"
        _judge(program, [err for _, _, err in _plain(program)])
    steps = [0, 0, 0]
    for _, out, _ in _plain("emu_ntt"):
        m = re.search(r"tiles stepped: one-step (\d+), two-step (\d+), three-step (\d+)", out)
        steps = [a + int(b) for a, b in zip(steps, m.groups())]
    assert all(steps), "one-, two- and three-step shapes must all have run under the contracts"


def test_the_contract_build_changes_no_output_of_emu_deep():
    """stdout of a contract build is the plain build's, word for word (one program stands for the mechanism: the hooks only read)."""
    plain = os.path.join(EMU, "build", "emu_deep_plain")
    src = os.path.join(EMU, "emu_deep.cpp")
    if _stale(plain, [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-o", plain, src])
    res = subprocess.run([plain], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout == _plain("emu_deep")[0][1] and "CONTRACT" not in res.stderr


# ---- saturated operands: the programs' printed records, recomputed here ----
def _records(out, tail=2):
    lines = out.split("\n")
    assert lines[-2] == "DONE", lines[-3:]
    return [l.split() for l in lines[:-tail]]


def test_saturated_transforms_and_the_ext_fold_match_the_oracle():
    out, err = _saturated("emu_ntt")
    assert "ALL OK" in out and len(re.findall(r"^saturated S\d+ failures=0$", out, re.M)) == len([a for a in SATURATED["emu_ntt"] if a[0] == "S"]), out[-2000:]
    m = re.search(r"tiles stepped: one-step (\d+), two-step (\d+), three-step (\d+)", out)
    assert m and all(int(g) > 0 for g in m.groups()), "every pass family must have stepped saturated tiles"
    _judge("emu_ntt", [err])


def test_saturated_deep_combination_and_evaluation():
    out, err = _saturated("emu_deep")
    recs, k, seen_t, polys = _records(out), 0, set(), 0
    while k < len(recs):
        r = recs[k]
        if r[0] == "DEEP":
            n, log_b, shift, z, width, stride, nterms, off = map(int, r[1:])
            terms = [tuple(map(int, recs[k + 1 + t][1:])) for t in range(nterms)]
            cols = np.array([list(map(int, recs[k + 1 + nterms + c][2:])) for c in range(width)], dtype=np.uint64)
            got = np.array(list(map(int, recs[k + 1 + nterms + width][1:])), dtype=np.uint32)
            assert (cols == P - 1).all() and all(a == SAT_X and v == SAT_X for _, _, a, v in terms)
            assert (got == deep_model(cols, terms, 1 << log_b, shift, z)).all(), (n, log_b, nterms)
            seen_t.add((nterms, log_b))
            k += 2 + nterms + width
        else:
            assert r[0] == "POLY"
            ncoeffs, stride, batch, npoints = map(int, r[1:5])
            points = list(map(int, r[5:]))
            got = list(map(int, recs[k + 1 + batch][1:]))
            assert points == [SAT_X, P - 1]
            for b in range(batch):
                coeffs = list(map(int, recs[k + 1 + b][2:]))
                assert coeffs == [P - 1] * ncoeffs
                for j, pt in enumerate(points):
                    acc = 0
                    for c in reversed(coeffs):
                        acc = (acc * pt + c) % P
                    assert got[b * npoints + j] == acc, (ncoeffs, b, j)
            polys += 1
            k += 2 + batch
    assert seen_t == {(t, b) for t in (4, 5, 8, 64, 65) for b in (0, 2)} and polys == 2
    _judge("emu_deep", [err])


def test_saturated_ext_deep_combination_and_evaluation():
    out, err = _saturated("emu_deep_ext")
    recs, k, seen_t, polys = _records(out), 0, set(), 0
    while k < len(recs):
        r = recs[k]
        if r[0] == "DEEPX":
            n, log_b, shift, z0, z1, z2, z3, width, stride, nterms, off = map(int, r[1:])
            terms = []
            for t in range(nterms):
                v = list(map(int, recs[k + 1 + t][1:]))
                terms.append((v[0], v[1], tuple(v[2:6]), tuple(v[6:10])))
                assert v[2:10] == [SAT_X] * 8
            cols = np.array([list(map(int, recs[k + 1 + nterms + c][2:])) for c in range(width)], dtype=np.uint64)
            got = np.array(list(map(int, recs[k + 1 + nterms + width][1:])), dtype=np.uint32).reshape(n, 4)
            assert (cols == P - 1).all()
            assert (got == em.deep_ext_model(cols, terms, 1 << log_b, shift, (z0, z1, z2, z3))).all(), (n, log_b, nterms)
            seen_t.add((nterms, log_b))
            k += 2 + nterms + width
        else:
            assert r[0] == "POLYX"
            ncoeffs, stride, batch, npoints = map(int, r[1:5])
            pts = list(map(int, r[5:]))
            points = [tuple(pts[4 * j:4 * j + 4]) for j in range(npoints)]
            assert points == [(SAT_X,) * 4, (P - 1,) * 4]
            got = np.array(list(map(int, recs[k + 1 + batch][1:])), dtype=np.uint32).reshape(batch, npoints, 4)
            columns = [list(map(int, recs[k + 1 + b][2:])) for b in range(batch)]
            assert all(c == [P - 1] * ncoeffs for c in columns)
            assert (got == em.poly_eval_ext_batch_model(columns[:1], points)[0]).all(), ncoeffs      # the columns are equal: one model run
            polys += 1
            k += 2 + batch
    assert seen_t == {(t, b) for t in (4, 5, 8, 64, 65) for b in (0, 2)} and polys == 2
    _judge("emu_deep_ext", [err])


def test_saturated_air_program():
    out, err = _saturated("emu_air")
    recs, k, cases = _records(out), 0, 0
    while k < len(recs):
        n, log_b, shift, nmats, ninsns, nweights, nregs = map(int, recs[k][1:])
        assert recs[k][0] == "AIR" and nmats == 1 and shift == SAT_X
        width = int(recs[k + 1][2])
        mats = [np.stack([np.array(recs[k + 2 + c][3:], dtype=np.uint64) for c in range(width)])]
        assert (mats[0] == P - 1).all()
        k += 2 + width
        insns = [tuple(map(int, recs[k + t][1:])) for t in range(ninsns)]
        assert (1, 1, 0, 0, SAT_X) in insns                                      # CONST SAT_X
        weights = list(map(int, recs[k + ninsns][1:]))
        assert weights == [SAT_X] * nweights
        got_c, got_q = np.array(recs[k + ninsns + 1][1:], dtype=np.uint32), np.array(recs[k + ninsns + 2][1:], dtype=np.uint32)
        want_c, want_q = air_model(insns, mats, n, log_b, shift, weights)
        assert (got_c == want_c).all() and (got_q == want_q).all(), (n, log_b)
        assert got_c.any() and got_q.any()
        k += ninsns + 3
        cases += 1
    assert cases == 4
    _judge("emu_air", [err])


def test_saturated_ext_scans():
    out, err = _saturated("emu_scan_ext")
    lines = out.split("\n")
    assert lines[-2] == "DONE" and lines[-3] == "BAD 0"
    recs, k, seen = [l.split() for l in lines[:-3]], 0, set()
    while k < len(recs):
        r = recs[k]
        if r[0] == "SCAN":
            op, n, batch, nw, dw, inplace, off, ns, ds, os_ = map(int, r[1:])
            init = list(map(int, recs[k + 1][1:]))
            nshift, dshift = tuple(map(int, recs[k + 2][1:])), tuple(map(int, recs[k + 3][1:]))
            assert nshift == ((SAT_X,) * 4 if nw else (0,) * 4) and dshift == ((SAT_X,) * 4 if dw else (0,) * 4) and init == [SAT_X] * (4 * batch)
            k += 4
            cols = []
            for b in range(batch):
                num = [list(map(int, recs[k + c][3:])) for c in range(nw)]
                den = [list(map(int, recs[k + nw + c][3:])) for c in range(dw)]
                assert all(c == [P - 1] * n for c in num + den)
                cols.append((num, den))
                k += nw + dw
            for b, (num, den) in enumerate(cols):
                got = [list(map(int, recs[k + c][3:])) for c in range(4)]
                tot = list(map(int, recs[k + 4][2:]))
                k += 5
                want, total, zeros, _ = test_emu_scan_ext.model(op, n, num, nw, nshift, den, dw, dshift, init[4 * b:4 * b + 4])
                assert all(got[c] == [w[c] for w in want] for c in range(4)), (op, n, nw, dw, b)
                assert tot == list(total) + [zeros, 0, 0, 0] and zeros == 0
            seen.add((op, n > test_emu_scan_ext.TILE, nw, dw))
        else:
            assert r[0] == "BINV"
            count = int(r[1])
            vin = [list(map(int, recs[k + 1 + c][3:])) for c in range(4)]
            vout = [list(map(int, recs[k + 5 + c][3:])) for c in range(4)]
            elems = [tuple(v[i] for v in vin) for i in range(count)]
            assert set(elems) == {(P - 1,) * 4, (SAT_X,) * 4}
            assert [tuple(v[i] for v in vout) for i in range(count)] == [em.inverse(e) for e in elems]
            k += 10
    assert seen == {(op, big, nw, dw) for op in (0, 1) for big in (False, True) for nw, dw in ((4, 4), (1, 1), (4, 0), (0, 4))}
    _judge("emu_scan_ext", [err])


def test_saturated_ext_fold_and_commit():
    out, err = _saturated("emu_fold_ext_commit")
    lines = out.split("\n")
    assert lines[-2] == "DONE" and len(lines) == 2 * 12 + 2
    for line in lines[:-2]:
        f = line.split()
        salted = int(f[0])
        a, b, x, beta = [int(v) for v in f[1:5]], [int(v) for v in f[5:9]], int(f[9]), [int(v) for v in f[10:14]]
        salt, folded, digest_hex = bytes.fromhex(f[14]), [int(v) for v in f[15:19]], f[19]
        assert beta == [SAT_X] * 4 and set(a + b) <= {0, P - 1}
        want = oracle.fri_fold_ext(np.array([a, b], dtype=np.uint64), np.array([x], dtype=np.uint64), np.array(beta, dtype=np.uint64))
        assert folded == [int(v) for v in want[0]], line
        leaf = rc.leaves_of(np.array([folded], dtype=np.uint64), np.frombuffer(salt, dtype=np.uint8).reshape(1, 16) if salted else None)[0]
        assert rc.hash_leaf(leaf).hex() == digest_hex, line
    _judge("emu_fold_ext_commit", [err])


# ---- the __global__ functions themselves ----
@lru_cache(maxsize=None)
def _sim_runs():
    """Plain runs of both tests/sim drivers, one process per kernel as their own tests run them, and of sim_pointwise."""
    jobs = [("sim_kernels", k) for k in sorted(test_sim_schedules.SITES, key=lambda k: ("pass3" not in k, "ntt" not in k))] + \
           [("sim_scan_ext", k) for k in test_sim_scan_ext.SITES] + [("sim_pointwise", None)]
    for p in ("sim_kernels", "sim_scan_ext", "sim_pointwise"):
        build_contracts(p)
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        return dict(zip(jobs, ex.map(lambda j: _run(j[0], ["--only", j[1]] if j[1] else []), jobs)))


def test_both_sim_drivers_keep_every_operand_domain():
    runs = _sim_runs()
    for program in ("sim_kernels", "sim_scan_ext"):
        mine = {k: v for (p, k), v in runs.items() if p == program}
        for k, (rc_, out, err) in mine.items():
            assert rc_ == 0 and "ALL OK" in out and "hard failures=0" in out, "%s --only %s:\n%s" % (program, k, (out + err)[-3000:])
            assert len(re.findall(r"^SCHEDULE \S+ failures=0$", out, re.M)) == 8, k
        _judge(program, [err for _, _, err in mine.values()])


def test_pointwise_kernels_match_the_oracle_and_keep_every_operand_domain():
    rc_, out, err = _sim_runs()[("sim_pointwise", None)]
    assert rc_ == 0 and "ALL OK" in out and "hard failures=0" in out, (out + err)[-3000:]
    ran = "\n".join(l for l in out.splitlines() if l.startswith("RAN "))
    for kernel in POINTWISE_KERNELS:
        assert re.search(r"^RAN " + kernel + r"(<|$)", ran, re.M), kernel + " never ran"
        assert kernel not in test_sim_schedules.SITES and kernel not in test_sim_scan_ext.SITES       # they have no synchronisation site
    for pattern in POINTWISE_INSTANTIATIONS:
        assert re.search(r"^RAN " + pattern, ran, re.M), "no instantiation matching " + pattern + "\n" + ran
    assert not re.search(r"^SITE ", out, re.M)
    _judge("sim_pointwise", [err])


def test_pointwise_only_runs_one_kernel_alone():
    """`--only K` runs the cases of K and reports nothing else as run; its contract lines are K's alone."""
    rc_, out, err = _run("sim_pointwise", ["--only", "domain_elements_kernel"])
    assert rc_ == 0 and re.findall(r"^RAN (\w+)", out, re.M) == ["domain_elements_kernel"]
    lines = contract_lines(err)
    assert lines["mont_mul"][0] > 0 and lines["wide_acc"][0] == 0


# ---- the harness has teeth ----
SELFTEST_TOYS = {
    "lazy_result_into_bb_add": "bb_add",
    "reduce_2p_of_2p": "bb_reduce_2p",
    "any_u32_times_lazy": "mont_mul_lazy",
    "any_u32_times_lazy_through_mont_mul": "mont_mul_lazy,mont_mul",
    "dot_sub_zero_twiddle": "mont_dot_sub",
    "dot_sub_wrong_negation": "mont_dot_sub",
    "dot2_lazy_factor": "mont_dot2",
    "five_saturated_products": "wide_acc",
    "wide_acc_lazy_factor": "wide_acc",
    "halve_of_p": "bb_halve",
    "sub_lazy_of_lazy": "bb_sub_lazy",
    "well_formed_saturated": "none",
    "transform_well_formed": "none",
    "fold_well_formed": "none",
}


def test_every_contract_binary_flags_each_toy_under_its_own_primitive():
    programs = list(EMU_PROGRAMS) + ["sim_kernels", "sim_scan_ext", "sim_pointwise"]
    for p in programs:
        build_contracts(p)
    with ThreadPoolExecutor(max_workers=WORKERS) as ex:
        results = list(ex.map(lambda p: _run(p, ["--contract-selftest"], timeout=120), programs))
    for program, (rc_, out, err) in zip(programs, results):
        assert rc_ == 0 and "CONTRACT SELFTEST OK" in out, program + ":\n" + out[-3000:] + err[-1000:]
        toys = dict(re.findall(r"^TOY (\w+) flagged=(\S+) violations=\d+ ok$", out, re.M))
        assert toys == SELFTEST_TOYS, (program, toys)
        # what the gap was: p in place of 0 is named by bb_add / bb_sub -- whether or not a word of the output moved (printed, not judged)
        for toy in ("transform_with_p_for_0", "fold_with_p_for_0"):
            m = re.search(r"^TOY %s flagged=(\S+) outputs (equal|differ from) the integer \w+ \(printed, not judged\)$" % toy, out, re.M)
            assert m and set(m.group(1).split(",")) <= {"bb_add", "bb_sub"} and m.group(1), (program, toy, out[-1500:])
        assert "CONTRACT bb_add" not in err, "the self-test replaces the run: no report of a run"


def test_a_violation_is_reported_with_operands_and_tag():
    """The report format end to end, on the header alone: a program whose one case feeds a lazy value to bb_add."""
    src = os.path.join(EMU, "build", "contract_probe.cpp")
    out = os.path.join(EMU, "build", "contract_probe_contracts")
    os.makedirs(os.path.dirname(src), exist_ok=True)
    with open(src, "w") as f:
        f.write('#include "bb_field.hpp"\n#include <cstdio>\nint main() {\n    TOYNI_CONTRACT_TAG("probe case=%d", 7);\n'
                '    std::printf("%u\\n", toyni::bb_add(toyni::BB_P + 5u, 1u));\n    return 0;\n}\n')
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-include", HEADER, "-o", out, src])
    res = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout == "6\n"
    lines = contract_lines(res.stderr)
    assert lines["bb_add"] == (1, 1, "first: %d 1 tag=probe case=7" % (P + 5)), res.stderr
    assert all(v == 0 for p, (_, v, _) in lines.items() if p != "bb_add")


def test_the_hook_is_inert_in_product_builds():
    """bb_field.hpp defines the hook as nothing unless a translation unit defined it first, and as nothing in device code whatever was
    defined; no product source defines it."""
    text = open(os.path.join(CSRC, "bb_field.hpp")).read()
    assert re.search(r"#if defined\(__HIP_DEVICE_COMPILE__\)\n#undef TOYNI_FIELD_CONTRACT\n#define TOYNI_FIELD_CONTRACT\(prim, \.\.\.\) \(\(void\)0\)\n"
                     r"#elif !defined\(TOYNI_FIELD_CONTRACT\)\n#define TOYNI_FIELD_CONTRACT\(prim, \.\.\.\) \(\(void\)0\)\n#endif", text)
    for folder, _, files in os.walk(os.path.join(ROOT, "toyni_amd")):
        for name in files:
            if name.endswith((".hpp", ".hip", ".h", ".py", ".cpp")) and name != "bb_field.hpp":
                assert "define TOYNI_FIELD_CONTRACT" not in open(os.path.join(folder, name), errors="replace").read(), name
    assert "field_contracts" not in open(os.path.join(ROOT, "__graft_entry__.py")).read()
