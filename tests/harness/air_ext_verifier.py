"""CPU verifier of the staged AIR proof under Ext challenges -- TEST INFRASTRUCTURE.  Python integers, the scalar functions of
tests/ext_model.py (Ext = F_p[X]/(X^4 - 11), an element a tuple of four residues) and hashlib: none of the numpy models the provers are
built from, nothing from the library.  The transcript, root_of_unity and inv are fib_verifier.py's, the record split and the Merkle rule
tests/rows_common.py's, the Ext fold of one pair fri_ext_verifier.fold_pair.  (fri_ext_verifier._open is not used: it names a wrong
salt, padding and position byte alike, and here each has a name of its own.)

Statement.  A main trace of four columns a, b, u, w over n rows: b is a permutation of a, and (u, w) is a LogUp pair that closes,
sum_i u_i / (gamma + w_i) = 0.  Both hold with overwhelming probability exactly when the accumulators below return to where they began.

    Z(g x) (gamma + b(x)) = Z(x) (gamma + a(x))              constraint 0, divided by Z_H = x^n - 1          g = w_n
    (S(g x) - S(x)) (gamma + w(x)) = u(x)                    constraint 1, divided by Z_H
    (Z(x) - 1) / (x - 1)                                     constraint 2, undivided
    S(x) / (x - 1)                                           constraint 3, undivided

Z and S are Ext-valued columns, each held as FOUR base columns, one per coordinate: Z(x) = sum_k X^k Z_k(x).  Every polynomial that is
committed or evaluated is a base-field one; gamma, the weights, z and every value at z are Ext.  An Ext challenge is four consecutive
squeeze_challenge values c0..c3; an Ext value is absorbed word by word (absorb_field of c0..c3).

  1. main         the 4 x N LDE of the columns on 7 <w_N>, N = n B, under ONE salted row tree (leaf = salt || a_i || b_i || u_i || w_i, 8 LE
                  bytes per value); absorb its root
  2. accumulators gamma = an Ext squeeze.  Z_0 = 1, Z_(i+1) = Z_i (gamma + a_i) / (gamma + b_i); S_0 = 0, S_(i+1) = S_i + u_i / (gamma + w_i).
                  One 8 x n matrix, coordinate-major: column k is Z_k, column 4 + k is S_k.  Its 8 x N LDE under one salted row tree
                  of width 8; absorb its root
  3. quotient     four Ext weights al_0..al_3; q = (al_0 e_0 + al_1 e_1) / Z_H + al_2 e_2 + al_3 e_3 on the coset, Ext-valued, held as
                  four base columns q_0..q_3 under one salted row tree of width 4; absorb its root
  4. z            an Ext squeeze, squeezed again while z_1 = z_2 = z_3 = 0 (such a z lies in no base-field set: not on the coset, not
                  in H, not 1).  Out-of-domain values, each an Ext element: "ood_main" the four main columns at z; "ood_acc" the eight
                  accumulator columns at z and at g z, column by column (column c at z is entry 2 c, at g z entry 2 c + 1); "ood_q" the
                  four q_j at z.  All absorbed in that order.  "q_z" = sum_j X^j q_j(z) travels too (derived, not absorbed)
  5. DEEP         one Ext weight per term, 4 + 16 + 4 squeezes in the order of the values above; with M the main, accumulator and quotient
                  matrices, d_i = sum_t w_t (M_t(i + rotation_t B) - value_t) / (x_i - z), rotation 1 for the values at g z: N Ext elements,
                  committed as rows of width 4 (leaf = salt || Ext::to_bytes); absorb the root
  6. FRI          log2 n Ext folds down to B elements; per fold squeeze an Ext beta, absorb the folded layer's root.  Layer k lives on
                  7^(2^k) <w_(N / 2^k)>.  The last layer is unsalted and sent in the clear
  7. queries      squeeze_indices(8, N / 2); a query i opens main row i, accumulator rows i and (i + B) mod N, quotient row i, DEEP rows
                  i and i + N / 2, the pair of every folded layer but the last

The proof is read in its wire form: the opening records as the device writes them (include/toyni_hip.h 3d: depth x 32 path bytes | 16
salt bytes | width x 8 value bytes | depth position bytes | zero padding to a multiple of 8), back to back in the order above.

verify(proof, why=None) checks, in this order: the shape of the proof, the ranges of its values, every Merkle path against its root
(along the positions the record itself states), q_z against the q_j(z) and the constraints at z against it, that the opened leaves are
the ones the transcript asks for, that the DEEP value of every query follows from the opened rows, every fold against the opened pair,
the final layer.  `why` (optional list) receives the name of the first check that failed."""
import ext_model as em
import rows_common as rc

from .fib_verifier import COSET_SHIFT, P, Transcript, root_of_unity
from .fri_ext_verifier import fold_pair

NUM_QUERIES = 8
MAIN_WIDTH, ACC_WIDTH, Q_WIDTH = 4, 8, 4
NUM_WEIGHTS = 4
# (matrix, column, rotation) of every DEEP term, in the order of the out-of-domain values and of the weights
DEEP_TERMS = ([("main", c, 0) for c in range(MAIN_WIDTH)] + [("acc", c, r) for c in range(ACC_WIDTH) for r in (0, 1)]
              + [("quotient", j, 0) for j in range(Q_WIDTH)])
BASIS = ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1))


def squeeze_ext(tr):
    return tuple(tr.squeeze_challenge() for _ in range(4))


def absorb_ext(tr, v):
    for c in v:
        tr.absorb_field(c)


def derive_z(tr):
    while True:
        z = squeeze_ext(tr)
        if any(z[1:]):
            return z


def from_columns(vals):
    """sum_k X^k v_k: the Ext value of an Ext column held as four base columns, from the four columns' (Ext) values at an Ext point."""
    acc = em.ZERO
    for k in range(4):
        acc = em.add(acc, em.mul(BASIS[k], tuple(vals[k])))
    return acc


def record_bytes(n, width):
    d = rc.depth_of(n)
    return 32 * d + 16 + 8 * width + ((d + 7) & ~7)


def opening_plan(N, B, n, qidx):
    """The opening groups of a proof in wire order: (name, tree leaves, leaf width, indices)."""
    groups = [("main", N, MAIN_WIDTH, list(qidx)),
              ("acc", N, ACC_WIDTH, [i for q in qidx for i in (q, (q + B) % N)]),
              ("quotient", N, Q_WIDTH, list(qidx)),
              ("deep", N, 4, [i for q in qidx for i in (q, q + N // 2)])]
    cur = list(qidx)
    for k in range(1, n.bit_length() - 1):
        half = (N >> k) // 2
        cur = [c % half for c in cur]
        groups.append((f"fri{k}", N >> k, 4, [i for c in cur for i in (c, c + half)]))
    return groups


def constraints_at(z, n, gamma, ood_main, ood_acc):
    """e_0 .. e_3 at z (the last two without their 1 / (z - 1)) from the out-of-domain values."""
    A, Bv, U, W = (tuple(v) for v in ood_main)
    Z, Zn = (from_columns([ood_acc[2 * k + r] for k in range(4)]) for r in (0, 1))
    S, Sn = (from_columns([ood_acc[2 * (4 + k) + r] for k in range(4)]) for r in (0, 1))
    e0 = em.sub(em.mul(Zn, em.add(gamma, Bv)), em.mul(Z, em.add(gamma, A)))
    e1 = em.sub(em.mul(em.sub(Sn, S), em.add(gamma, W)), U)
    return e0, e1, em.sub(Z, em.ONE), S


def quotient_at(z, n, alphas, e):
    zh_inv, x1_inv = em.inverse(em.sub(em.power(z, n), em.ONE)), em.inverse(em.sub(z, em.ONE))
    return em.add(em.mul(em.add(em.mul(alphas[0], e[0]), em.mul(alphas[1], e[1])), zh_inv),
                  em.mul(em.add(em.mul(alphas[2], e[2]), em.mul(alphas[3], e[3])), x1_inv))


def _ext_list(vals, count):
    out = [tuple(int(c) for c in v) for v in vals]
    if len(out) != count or any(len(v) != 4 for v in out):
        return None
    return out


def verify(proof, why=None):
    def fail(name):
        if why is not None:
            why.append(name)
        return False

    # ---- 0. shape, ranges ----
    n, N = proof["trace_len"], proof["lde_size"]
    if n < 2 or n & (n - 1) or N < 2 * n or N % n or (N // n) & (N // n - 1) or N.bit_length() - 1 > 27:
        return fail("sizes")
    B = N // n
    folds = n.bit_length() - 1
    w_N = root_of_unity(N.bit_length() - 1)
    ood_main, ood_acc, ood_q = _ext_list(proof["ood_main"], MAIN_WIDTH), _ext_list(proof["ood_acc"], 2 * ACC_WIDTH), _ext_list(proof["ood_q"], Q_WIDTH)
    q_z = _ext_list([proof["q_z"]], 1)
    if ood_main is None or ood_acc is None or ood_q is None or q_z is None:
        return fail("ood_shape")
    q_z = q_z[0]
    commitments = [bytes(c) for c in proof["fri_commitments"]]
    if len(commitments) != folds + 1:
        return fail("fold_count")
    final = _ext_list(proof["fri_final_layer"], B)
    if final is None:
        return fail("final_size")
    if any(not 0 <= c < P for v in ood_main + ood_acc + ood_q + [q_z] + final for c in v):
        return fail("value_range")

    # ---- the transcript ----
    roots = {k: bytes(proof[k + "_commitment"]) for k in ("main", "acc", "quotient")}
    tr = Transcript()
    tr.absorb(roots["main"])
    gamma = squeeze_ext(tr)
    tr.absorb(roots["acc"])
    alphas = [squeeze_ext(tr) for _ in range(NUM_WEIGHTS)]
    tr.absorb(roots["quotient"])
    z = derive_z(tr)
    ood = ood_main + ood_acc + ood_q
    for v in ood:
        absorb_ext(tr, v)
    deep_w = [squeeze_ext(tr) for _ in DEEP_TERMS]
    tr.absorb(commitments[0])
    betas = []
    for c in commitments[1:]:
        betas.append(squeeze_ext(tr))
        tr.absorb(c)
    qidx = tr.squeeze_indices(NUM_QUERIES, N // 2)

    # ---- 1. every opening against its root, along the positions its own record states ----
    plan = opening_plan(N, B, n, qidx)          # the counts and sizes depend on n and N alone; the indices are held against step 3
    raw = bytes(memoryview(proof["opening_records"]))
    if len(raw) != sum(len(ix) * record_bytes(t, w) for _, t, w, ix in plan):
        return fail("record_length")
    roots["deep"] = commitments[0]
    roots.update({f"fri{k}": commitments[k] for k in range(1, folds)})
    records = {}
    off = 0
    for name, t, w, ix in plan:
        rec, d = record_bytes(t, w), rc.depth_of(t)
        kind = name if not name.startswith("fri") else "fri"
        for k in range(len(ix)):
            r = raw[off:off + rec]
            off += rec
            path, salt, vals, flags, pad = rc.split_record(r, t, w)
            if any(pad):
                return fail(kind + "_padding")
            if any(f > 1 for f in r[rec - len(pad) - d:rec - len(pad)]):
                return fail(kind + "_position")
            values = [int.from_bytes(vals[8 * c:8 * c + 8], "little") for c in range(w)]
            if any(v >= P for v in values):
                return fail("value_range")
            if not rc.verify_merkle_proof(salt + vals, path, flags, roots[name]):
                return fail(kind + "_merkle")
            records[name, k] = (sum(int(f) << l for l, f in enumerate(flags)), values)    # the leaf the path belongs to (trees of 2^d leaves)

    # ---- 2. the constraints at z ----
    if q_z != from_columns(ood_q):
        return fail("q_recombination")
    if q_z != quotient_at(z, n, alphas, constraints_at(z, n, gamma, ood_main, ood_acc)):
        return fail("ood")

    # ---- 3. the queries the transcript asks for: the opened leaves are those, and the DEEP value follows from the opened rows ----
    if [int(i) for i in proof["query_indices"]] != qidx:
        return fail("query_index")
    claimed = [(int(t), int(w), bool(s), [int(i) for i in ix]) for t, w, s, ix in proof["opening_groups"]]
    if claimed != [(t, w, True, ix) for _, t, w, ix in plan]:
        return fail("opening_groups")
    opened = {}
    for name, _, _, ix in plan:
        for k, i in enumerate(ix):
            if records[name, k][0] != i:
                return fail((name if not name.startswith("fri") else "fri") + "_index")
            opened[name, i] = records[name, k][1]
    for qi in qidx:
        x_i = COSET_SHIFT * pow(w_N, qi, P) % P
        num = em.ZERO
        for (mat, c, r), wt, val in zip(DEEP_TERMS, deep_w, ood):
            cell = opened[mat, (qi + r * B) % N][c]
            num = em.add(num, em.mul(wt, em.sub(em.embed(cell), val)))
        if tuple(opened["deep", qi]) != em.mul(num, em.inverse(em.sub(em.embed(x_i), z))):
            return fail("deep_value")

    # ---- 4. every fold from the opened pair (layer k lives on 7^(2^k) <w_(N / 2^k)>) ----
    last_fold = []
    for qi in qidx:
        x_i = COSET_SHIFT * pow(w_N, qi, P) % P
        prev = fold_pair(tuple(opened["deep", qi]), tuple(opened["deep", qi + N // 2]), x_i, betas[0])
        pos = qi
        for k in range(1, folds):
            half = (N >> k) // 2
            lo = pos % half
            if tuple(opened[f"fri{k}", pos]) != prev:
                return fail("fri_consistency")
            x = pow(COSET_SHIFT * pow(w_N, lo, P) % P, 1 << k, P)
            prev = fold_pair(tuple(opened[f"fri{k}", lo]), tuple(opened[f"fri{k}", lo + half]), x, betas[k])
            pos = lo
        last_fold.append((pos, prev))

    # ---- 5. the final layer: B equal elements under the last commitment (unsalted rows of width 4), and what the last fold gave ----
    if any(v != final[0] for v in final):
        return fail("final_not_constant")
    leaves = [b"".join(c.to_bytes(8, "little") for c in v) for v in final]
    if rc.hashlib_levels(leaves)[-1][0] != commitments[-1]:
        return fail("final_commitment")
    if any(final[pos] != prev for pos, prev in last_fold):
        return fail("final_value")
    return True
