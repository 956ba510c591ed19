"""Oracle-only prover of the staged AIR proof under Ext challenges -- TEST INFRASTRUCTURE.  The protocol of air_ext_verifier.py, computed
with nothing but the C oracle (oracle/: intt, domain_fft, domain_ifft, fri_fold_ext), tests/ext_model.py, hashlib trees
(air_ref_prover.Tree) and the transcript of fib_verifier.py.  No device code is involved, no constraint program and no instruction
list: the scans are a loop over Python Ext elements, the constraints are written out in Ext with ext_model.vmul on the LDE arrays, the
DEEP layer is ext_model.deep_ext_model, one call per matrix, summed.  A proof computed here is what the device prover
(air_ext_prover.py) must emit on the same trace and seed, byte for byte -- the serialized opening records included, padding zero.

    proof, components = prove(main, log_blowup, seed)

  proof       the fields air_ext_verifier.verify reads (WIRE_FIELDS)
  components  the intermediate values, for a test that wants to say where two provers part

The salts are numpy's default_rng(seed) bytes, 16 per leaf, in the order main tree, accumulator tree, quotient tree, DEEP tree, then
every salted folded layer from the largest down (salt_pool); the device prover uploads the same pool as it is.

scalar=True takes the slow forms throughout (one Ext inversion per scan term, Horner in Python for every out-of-domain value, pow() per
point for 1 / Z_H and 1 / (x - 1)); the default inverts the scan's denominators behind one inversion (ext_model.batch_inverse),
evaluates through a table of powers of the point and raises whole arrays to p - 2.  tests/test_air_ext_harness.py holds the two equal.

`cheat` (tests only) makes a dishonest prover, one deviation per key, everything after it computed as the protocol says:
  "weight_coordinates_transposed": True   coordinate c of the quotient takes coordinate j of a constraint by (al X^c)_j, not (al X^j)_c
  "gamma_reversed": True                  the scans use (gamma_3, gamma_2, gamma_1, gamma_0)
  "acc_coordinate_minor": True            the accumulator matrix is committed (evaluated, combined) with the columns of Z and S interleaved
  "q_z_without_powers": True              q_z = sum_j q_j(z)
  "swap_z_gz": True                       the values of Z at z and at g z change places
  "drop_q_terms": True                    the DEEP sum without the quotient's matrix
  "overwrite_second_matrix": True         the DEEP sum is the accumulator matrix's terms and the quotient's: the main matrix's are lost
  "rotation_rows": r                      the second accumulator row of a query is opened at i + r instead of i + B
  "beta_reversed": True                   every fold uses (beta_3, beta_2, beta_1, beta_0)
  "tamper": f(name, layer)                may change a layer ("deep", "fri1", ...: (m, 4) residues) in place before it is committed"""
import numpy as np

import ext_model as em
import oracle

from . import air_ext_verifier as av
from .air_ext_verifier import ACC_WIDTH, DEEP_TERMS, MAIN_WIDTH, NUM_QUERIES, NUM_WEIGHTS, opening_plan, record_bytes
from .air_ref_prover import Tree, _record_field, layer_sizes
from .fib_verifier import COSET_SHIFT, P, Transcript, root_of_unity
from .ref_prover import _first_index

WIRE_FIELDS = ("trace_len", "lde_size", "main_commitment", "acc_commitment", "quotient_commitment", "ood_main", "ood_acc", "ood_q", "q_z",
               "fri_commitments", "fri_final_layer", "query_indices", "opening_groups", "opening_records")
_p = np.uint64(P)


def true_main(n, seed):
    """Columns a, b, u, w: b a permutation of a; rows 0 .. n/2 - 1 of (u, w) look values up (+1 / (gamma + v)), rows n/2 .. n - 1 hold the
    table with its multiplicities (-m / (gamma + t)), so the sum closes."""
    rng = np.random.default_rng(4000 + seed)
    a = rng.integers(0, P, n)
    b = a[rng.permutation(n)]
    t = np.unique(rng.integers(0, P, 4 * n))[:n // 2]
    assert t.size == n // 2
    picks = rng.integers(0, max(n // 8, 1), n // 2)
    m = np.bincount(picks, minlength=n // 2)
    u = np.concatenate([np.ones(n // 2, dtype=np.int64), (-m) % P])
    w = np.concatenate([t[picks], t])
    return np.array([a, b, u, w], dtype=np.uint64)


def salt_pool(n, N, seed):
    leaves = 4 * N + sum(layer_sizes(n, N)[:-1])
    return np.random.default_rng(seed).integers(0, 256, (leaves, 16), dtype=np.uint8)


# ---- Ext on arrays ----
def _embed(col, shift=em.ZERO):
    """(len, 4): the base column embedded in Ext, plus an Ext constant."""
    out = np.zeros((len(col), 4), dtype=np.uint64)
    out[:, 0] = col
    return (out + np.array(shift, dtype=np.uint64)) % _p


def _vsub(a, b):
    return (a + _p - b) % _p


def _vpow(base, e):
    """base^e element-wise in the base field (square and multiply on the whole array)."""
    base = np.asarray(base, dtype=np.uint64) % _p
    out = np.ones_like(base)
    while e:
        if e & 1:
            out = out * base % _p
        base = base * base % _p
        e >>= 1
    return out


def powers_of(point, count):
    """(count, 4): point^0 .. point^(count - 1), by doubling the table."""
    out = np.zeros((count, 4), dtype=np.uint64)
    out[0, 0] = 1
    have, step = 1, tuple(point)
    while have < count:
        take = min(have, count - have)
        out[have:have + take] = em.vmul(out[:take], np.array(step, dtype=np.uint64))
        have, step = have + take, em.mul(step, step)
    return out


def eval_columns(columns, points, scalar):
    """[column][point] -> Ext: base coefficients at Ext points."""
    if scalar:
        return [[em.poly_eval_ext(col, pt) for pt in points] for col in columns]
    tables = [powers_of(pt, columns.shape[1]) for pt in points]
    return [[tuple(int((col * t[:, k] % _p).sum() % _p) for k in range(4)) for t in tables] for col in np.asarray(columns, dtype=np.uint64)]


def scan(op, num, den, init, scalar):
    """out_0 = init, out_(i+1) = out_i (op) num_i / den_i over Python Ext elements -> (4, n): the four coordinate columns."""
    den_inv = [em.inverse(d) for d in den] if scalar else em.batch_inverse(den)
    out, acc = [], init
    for nu, di in zip(num, den_inv):
        out.append(acc)
        acc = op(acc, em.mul(nu, di))
    return np.array(out, dtype=np.uint64).T, acc


def _weigh(e, alpha, transposed):
    """alpha e for an (N, 4) array of Ext values.  transposed: the 4 x 4 matrix of "multiply by alpha" used the other way round."""
    if not transposed:
        return em.vmul(e, np.array(alpha, dtype=np.uint64))
    m = [em.mul(alpha, av.BASIS[j]) for j in range(4)]          # m[j][c] = (alpha X^j)_c; honest: out_c = sum_j m[j][c] e_j
    return np.stack([sum(e[:, j] * np.uint64(m[c][j]) % _p for j in range(4)) % _p for c in range(4)], axis=-1)


# ---- the prover ----
def prove(main, log_blowup, seed, cheat=None, scalar=False):
    cheat = cheat or {}
    main = np.asarray(main, dtype=np.uint64)
    assert main.ndim == 2 and main.shape[0] == MAIN_WIDTH
    n = main.shape[1]
    assert n >= 2 and n & (n - 1) == 0 and log_blowup >= 1
    B, N = 1 << log_blowup, n << log_blowup
    g = root_of_unity(n.bit_length() - 1)
    sizes = layer_sizes(n, N)
    pool = salt_pool(n, N, seed)
    taken = [0]

    def take_salts(count):
        s = pool[taken[0]:taken[0] + count]
        taken[0] += count
        return s

    tamper = cheat.get("tamper", lambda name, layer: None)
    lde_of = lambda coeffs: np.stack([oracle.domain_fft(c, N, COSET_SHIFT) for c in coeffs])

    # 1. the main columns: interpolate, extend to the coset, one row tree
    main_coeffs = np.stack([oracle.intt(c) for c in main])
    main_lde = lde_of(main_coeffs)
    main_tree = Tree(main_lde.T, take_salts(N))
    tr = Transcript()
    tr.absorb(main_tree.root)

    # 2. the accumulators under gamma: a loop over Ext elements; eight base columns, coordinate-major
    gamma = av.squeeze_ext(tr)
    gs = gamma[::-1] if cheat.get("gamma_reversed") else gamma
    a, b, u, w = ([int(v) for v in col] for col in main)
    plus = lambda col: [em.add(gs, em.embed(v)) for v in col]
    z_cols, z_total = scan(em.mul, plus(a), plus(b), em.ONE, scalar)
    s_cols, s_total = scan(em.add, [em.embed(v) for v in u], plus(w), em.ZERO, scalar)
    acc = np.concatenate([z_cols, s_cols])
    acc_lde = lde_of(np.stack([oracle.intt(c) for c in acc]))              # what the constraints read
    sent = acc[[0, 4, 1, 5, 2, 6, 3, 7]] if cheat.get("acc_coordinate_minor") else acc
    sent_coeffs = np.stack([oracle.intt(c) for c in sent])
    sent_lde = lde_of(sent_coeffs)                                         # what is committed, evaluated and combined
    acc_tree = Tree(sent_lde.T, take_salts(N))
    tr.absorb(acc_tree.root)

    # 3. the quotient under four Ext weights, the constraints written out on the LDE arrays
    alphas = [av.squeeze_ext(tr) for _ in range(NUM_WEIGHTS)]
    xs = oracle.domain_elements(N, COSET_SHIFT)
    zh_inv = _vpow(_vsub(_vpow(xs, n), np.uint64(1)), P - 2)[:, None]
    x1_inv = _vpow(_vsub(xs, np.uint64(1)), P - 2)[:, None]
    if scalar:
        zh_inv = np.array([pow(pow(int(x), n, P) - 1, P - 2, P) for x in xs], dtype=np.uint64)[:, None]
        x1_inv = np.array([pow(int(x) - 1, P - 2, P) for x in xs], dtype=np.uint64)[:, None]
    Zx, Sx = acc_lde[0:4].T, acc_lde[4:8].T
    Zg, Sg = np.roll(Zx, -B, axis=0), np.roll(Sx, -B, axis=0)
    la, lb, lu, lw = main_lde
    e = [_vsub(em.vmul(Zg, _embed(lb, gamma)), em.vmul(Zx, _embed(la, gamma))),
         _vsub(em.vmul(_vsub(Sg, Sx), _embed(lw, gamma)), _embed(lu)),
         _vsub(Zx, np.array(em.ONE, dtype=np.uint64)),
         Sx]
    t = cheat.get("weight_coordinates_transposed", False)
    q = ((_weigh(e[0], alphas[0], t) + _weigh(e[1], alphas[1], t)) % _p * zh_inv % _p
         + (_weigh(e[2], alphas[2], t) + _weigh(e[3], alphas[3], t)) % _p * x1_inv % _p) % _p
    q_lde = np.ascontiguousarray(q.T)                                      # q_0 .. q_3
    q_tree = Tree(q, take_salts(N))
    tr.absorb(q_tree.root)

    # 4. z and the out-of-domain values
    q_coeffs = np.stack([oracle.domain_ifft(c, COSET_SHIFT) for c in q_lde])
    z = av.derive_z(tr)
    gz = tuple(c * g % P for c in z)
    ood_main = [v[0] for v in eval_columns(main_coeffs, [z], scalar)]
    ood_acc = [v for pair in eval_columns(sent_coeffs, [z, gz], scalar) for v in pair]
    if cheat.get("swap_z_gz"):
        for c in range(4):
            ood_acc[2 * c], ood_acc[2 * c + 1] = ood_acc[2 * c + 1], ood_acc[2 * c]
    ood_q = [v[0] for v in eval_columns(q_coeffs, [z], scalar)]
    q_z = av.from_columns(ood_q)
    if cheat.get("q_z_without_powers"):
        q_z = em.ZERO
        for v in ood_q:
            q_z = em.add(q_z, v)
    ood = ood_main + ood_acc + ood_q
    for v in ood:
        av.absorb_ext(tr, v)

    # 5. the DEEP layer: one deep_ext_model call per matrix, summed
    deep_w = [av.squeeze_ext(tr) for _ in DEEP_TERMS]
    mats = {"main": main_lde, "acc": sent_lde, "quotient": q_lde}
    keep = [m for m in mats if not (m == "quotient" and cheat.get("drop_q_terms")) and not (m == "main" and cheat.get("overwrite_second_matrix"))]
    deep = np.zeros((N, 4), dtype=np.uint64)
    den = em.deep_denominators(N, COSET_SHIFT, z)                          # the three calls share 1 / (x_i - z)
    for m in keep:
        terms = [(c, r, wt, val) for (mat, c, r), wt, val in zip(DEEP_TERMS, deep_w, ood) if mat == m]
        deep = (deep + em.deep_ext_model(mats[m], terms, B, COSET_SHIFT, z, inv=den).astype(np.uint64)) % _p
    tamper("deep", deep)

    # 6. FRI: layer k lives on 7^(2^k) <w_(N / 2^k)>; beta_k is squeezed before the next root is absorbed; the last layer is unsalted
    layers = [deep]
    trees = [Tree(deep, take_salts(N))]
    tr.absorb(trees[0].root)
    betas = []
    shift = COSET_SHIFT
    for k, m in enumerate(sizes):
        betas.append(av.squeeze_ext(tr))
        used = betas[-1][::-1] if cheat.get("beta_reversed") else betas[-1]
        folded = oracle.fri_fold_ext(layers[-1], oracle.domain_elements(2 * m, shift), np.array(used, dtype=np.uint64))
        tamper(f"fri{k + 1}", folded)
        layers.append(folded)
        shift = shift * shift % P
        trees.append(Tree(folded, take_salts(m) if m != B else None))
        tr.absorb(trees[-1].root)

    # 7. queries
    qidx = tr.squeeze_indices(NUM_QUERIES, N // 2)
    plan = opening_plan(N, B, n, qidx)
    honest_plan = list(plan)                          # a cheating prover still claims the indices the verifier expects
    if "rotation_rows" in cheat:
        plan[1] = ("acc", N, ACC_WIDTH, [i for q_ in qidx for i in (q_, (q_ + cheat["rotation_rows"]) % N)])
    by_name = {"main": main_tree, "acc": acc_tree, "quotient": q_tree, "deep": trees[0]}
    by_name.update({f"fri{k}": trees[k] for k in range(1, len(sizes))})
    records = np.concatenate([by_name[name].records(ix) for name, _, _, ix in plan])
    proof = {
        "trace_len": n, "lde_size": N, "main_commitment": main_tree.root, "acc_commitment": acc_tree.root, "quotient_commitment": q_tree.root,
        "ood_main": ood_main, "ood_acc": ood_acc, "ood_q": ood_q, "q_z": q_z,
        "fri_commitments": [t_.root for t_ in trees], "fri_final_layer": [tuple(int(c) for c in v) for v in layers[-1]],
        "query_indices": qidx, "opening_groups": [(t_, w_, True, ix) for _, t_, w_, ix in honest_plan], "opening_records": records,
    }
    components = {"main_coeffs": main_coeffs, "main_lde": main_lde, "gamma": gamma, "acc": acc, "totals": (z_total, s_total), "acc_lde": sent_lde,
                  "alphas": alphas, "q_lde": q_lde, "q_coeffs": q_coeffs, "z": z, "ood": ood, "deep_weights": deep_w, "deep": deep,
                  "betas": betas, "fri_layers": layers[1:]}
    return proof, components


# ---- comparison: "" when equal, else the first difference in protocol order ----
def first_proof_difference(got: dict, want: dict) -> str:
    """Byte-exact comparison of two proofs in wire form (WIRE_FIELDS), field by field in protocol order; inside the opening records the
    first differing byte is named by group, record, leaf and field."""
    for key in ("trace_len", "lde_size"):
        if int(got[key]) != int(want[key]):
            return f"{key}: {int(got[key])} != {int(want[key])}"
    for key in ("main_commitment", "acc_commitment", "quotient_commitment"):
        if bytes(got[key]) != bytes(want[key]):
            return f"{key}: {bytes(got[key]).hex()} != {bytes(want[key]).hex()}"
    for key in ("ood_main", "ood_acc", "ood_q", "q_z"):
        msg = _first_index(f"{key} (words, four per value)", got[key], want[key])
        if msg:
            return msg
    gc, wc = got["fri_commitments"], want["fri_commitments"]
    if len(gc) != len(wc):
        return f"fri_commitments: {len(gc)} roots, want {len(wc)}"
    for k, (x, y) in enumerate(zip(gc, wc)):
        if bytes(x) != bytes(y):
            return f"fri_commitments[{k}] ({'DEEP layer' if k == 0 else f'after {k} folds'}): {bytes(x).hex()} != {bytes(y).hex()}"
    for key in ("fri_final_layer", "query_indices"):
        msg = _first_index(key, got[key], want[key])
        if msg:
            return msg
    gg = [(int(t), int(w), bool(s), [int(i) for i in ix]) for t, w, s, ix in got["opening_groups"]]
    wg = [(int(t), int(w), bool(s), [int(i) for i in ix]) for t, w, s, ix in want["opening_groups"]]
    if gg != wg:
        k = next((k for k, (x, y) in enumerate(zip(gg, wg)) if x != y), min(len(gg), len(wg)))
        return f"opening_groups[{k}] differ ({len(gg)} groups, want {len(wg)})"
    graw = np.asarray(got["opening_records"], dtype=np.uint8).reshape(-1)
    wraw = np.asarray(want["opening_records"], dtype=np.uint8).reshape(-1)
    if graw.size != wraw.size:
        return f"opening_records: {graw.size} bytes, want {wraw.size}"
    off = 0
    for k, (tn, width, _salted, ix) in enumerate(wg):
        rec, d = record_bytes(tn, width), av.rc.depth_of(tn)
        x, y = graw[off:off + rec * len(ix)], wraw[off:off + rec * len(ix)]
        bad = np.nonzero(x != y)[0]
        if bad.size:
            r, byte = divmod(int(bad[0]), rec)
            return (f"opening_records of group {k} (tree of {tn} leaves, {width} per leaf): record {r} (leaf {ix[r]}), byte {byte} of {rec} "
                    f"({_record_field(byte, d, width)}; {int(x[bad[0]])} != {int(y[bad[0]])}; {bad.size} bytes differ in the group)")
        off += rec * len(ix)
    return ""
