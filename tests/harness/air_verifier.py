"""CPU verifier of the two-column AIR proof -- TEST INFRASTRUCTURE.  Python integers and hashlib only: no numpy field arithmetic, none
of the models the provers are built from, nothing from the library.  The protocol is the one of the Fibonacci proof (fib_verifier.py,
whose transcript, derive_z, index squeezing and Merkle rules are imported) carried to a trace of two columns a, b over n rows:

    constraint 0 (divided by Z_H = x^n - 1)   (a(gx) - b(x)) (x - last)                 g = w_n, last = g^(n-1)
    constraint 1 (divided by Z_H)             (b(gx) - a(x) b(x) - 1) (x - last)
    constraint 2 (undivided)                  (a(x) - a_0) / (x - 1)
    constraint 3 (undivided)                  (b(x) - b_0) / (x - 1)

  transcript  absorb the trace root (ONE salted row tree over the 2 x N LDE on 7 <w_N>, N = n B; leaf = salt || a_i || b_i, 8 LE bytes
              per value), squeeze the four constraint weights, absorb the quotient root (salted single-column tree over q), derive z,
              absorb a(z), a(gz), b(z), b(gz), q(z), squeeze the five DEEP weights, absorb the DEEP root; per fold squeeze beta, absorb
              the folded layer's root; squeeze NUM_QUERIES indices below N / 2
  DEEP layer  d_i = (al_0 (a_i - a(z)) + al_1 (a_(i+B) - a(gz)) + al_2 (b_i - b(z)) + al_3 (b_(i+B) - b(gz)) + al_4 (q_i - q(z))) / (x_i - z)
  FRI         log2 n folds down to B values, sent in the clear (their unsalted tree is the last commitment)
  a query i   trace rows i and (i + B) mod N, q_i, d_i and d_(i + N/2), the pair of every folded layer but the last

The proof is read in its wire form: the opening records as the device writes them (include/toyni_hip.h 3c / 3d: depth x 32 path bytes |
16 salt bytes | width x 8 value bytes | depth position bytes | zero padding to a multiple of 8), back to back in the order trace rows,
quotient, DEEP layer, folded layers.  Which leaves they open is derived here, from the transcript; the position bytes must say so.

verify(proof, why=None) checks, in this order: the shape of the proof, every Merkle path against its root (along the positions the record
itself states), the constraints at z against q(z), that the opened leaves are the ones the transcript asks for and the DEEP value of
every query follows from the opened rows, every fold against the opened pair, the final layer.  `why` (optional list) receives the name
of the first check that failed.  (The leaves asked for depend on everything absorbed, the out-of-domain values included: held against
the records before the constraints at z, a wrong out-of-domain value would be reported as a wrong leaf.)"""
from .fib_verifier import COSET_SHIFT, P, Transcript, derive_z, inv, merkle_root_of, root_of_unity, verify_merkle_proof

NUM_QUERIES = 8
NUM_WEIGHTS, NUM_DEEP_WEIGHTS = 4, 5
OOD_KEYS = ("a_z", "a_gz", "b_z", "b_gz", "q_z")


def depth_of(n):
    d = 0
    while n > 1:
        n, d = (n + 1) // 2, d + 1
    return d


def record_bytes(n, width):
    """Bytes of one opening record of a tree of n leaves whose leaf holds `width` values."""
    d = depth_of(n)
    return 32 * d + 16 + 8 * width + ((d + 7) & ~7)


def opening_plan(N, B, n, qidx):
    """The opening groups of a proof in wire order: (name, tree leaves, leaf width, indices)."""
    groups = [("trace", N, 2, [i for q in qidx for i in (q, (q + B) % N)]),
              ("quotient", N, 1, list(qidx)),
              ("deep", N, 1, [i for q in qidx for i in (q, q + N // 2)])]
    cur = list(qidx)
    folds = n.bit_length() - 1
    for k in range(1, folds):
        half = (N >> k) // 2
        cur = [c % half for c in cur]
        groups.append((f"fri{k}", N >> k, 1, [i for c in cur for i in (c, c + half)]))
    return groups


def split_record(rec, n, width):
    """(path, salt, values, position flags, padding) of one record."""
    d = depth_of(n)
    path = [rec[32 * l:32 * l + 32] for l in range(d)]
    salt = rec[32 * d:32 * d + 16]
    at = 32 * d + 16
    values = [int.from_bytes(rec[at + 8 * c:at + 8 * c + 8], "little") for c in range(width)]
    flags = rec[at + 8 * width:at + 8 * width + d]
    return path, salt, values, flags, rec[at + 8 * width + d:]


def constraints_at(z, n, a_0, b_0, a_z, a_gz, b_z, b_gz):
    """The four constraint values at z from the trace's out-of-domain values."""
    last = pow(root_of_unity(n.bit_length() - 1), n - 1, P)
    iz1 = inv((z - 1) % P)
    return ((a_gz - b_z) * (z - last) % P, (b_gz - a_z * b_z - 1) * (z - last) % P, (a_z - a_0) * iz1 % P, (b_z - b_0) * iz1 % P)


def fold_pair(a, b, beta, x):
    """fri_fold at one point: (a + b) / 2 + (a - b) / 2 * beta / x."""
    half = inv(2)
    return ((a + b) * half + (a - b) * half % P * beta % P * inv(x)) % P


def verify(proof, why=None):
    def fail(name):
        if why is not None:
            why.append(name)
        return False

    # ---- 0. shape ----
    n, N = proof["trace_len"], proof["lde_size"]
    if n < 2 or n & (n - 1) or N < 2 * n or N % n or (N // n) & (N // n - 1) or N.bit_length() - 1 > 27:
        return fail("sizes")
    B = N // n
    folds = n.bit_length() - 1
    w_N = root_of_unity(N.bit_length() - 1)
    a_0, b_0 = proof["a_0"], proof["b_0"]
    ood = [proof[k] for k in OOD_KEYS]
    if any(not 0 <= v < P for v in ood + [a_0, b_0]):
        return fail("value_range")
    commitments = [bytes(c) for c in proof["fri_commitments"]]
    if len(commitments) != folds + 1:
        return fail("fold_count")
    final = [int(v) for v in proof["fri_final_layer"]]
    if len(final) != B:
        return fail("final_size")
    if any(not 0 <= v < P for v in final):
        return fail("value_range")

    # ---- the transcript ----
    tr = Transcript()
    tr.absorb(bytes(proof["trace_commitment"]))
    weights = [tr.squeeze_challenge() for _ in range(NUM_WEIGHTS)]
    tr.absorb(bytes(proof["quotient_commitment"]))
    z = derive_z(tr, N)
    for v in ood:
        tr.absorb_field(v)
    alphas = [tr.squeeze_challenge() for _ in range(NUM_DEEP_WEIGHTS)]
    tr.absorb(commitments[0])
    betas = []
    for c in commitments[1:]:
        betas.append(tr.squeeze_challenge())
        tr.absorb(c)
    qidx = tr.squeeze_indices(NUM_QUERIES, N // 2)

    # ---- 1. every opening against its root, along the positions its own record states ----
    plan = opening_plan(N, B, n, qidx)          # the counts and sizes depend on n and N alone; the indices are held against step 3
    raw = bytes(memoryview(proof["opening_records"]))
    if len(raw) != sum(len(ix) * record_bytes(t, w) for _, t, w, ix in plan):
        return fail("record_length")
    roots = {"trace": bytes(proof["trace_commitment"]), "quotient": bytes(proof["quotient_commitment"]), "deep": commitments[0]}
    roots.update({f"fri{k}": commitments[k] for k in range(1, folds)})
    records = {}
    off = 0
    for name, t, w, ix in plan:
        rec = record_bytes(t, w)
        kind = name if not name.startswith("fri") else "fri"
        for k in range(len(ix)):
            path, salt, values, flags, pad = split_record(raw[off:off + rec], t, w)
            off += rec
            if any(pad):
                return fail(kind + "_padding")
            if any(f > 1 for f in flags):
                return fail(kind + "_position")
            if any(v >= P for v in values):
                return fail("value_range")
            leaf = salt + b"".join(v.to_bytes(8, "little") for v in values)
            if not verify_merkle_proof(leaf, path, [bool(f) for f in flags], roots[name]):
                return fail(kind + "_merkle")
            records[name, k] = (sum(f << l for l, f in enumerate(flags)), values)    # the leaf the path belongs to (trees of 2^d leaves)

    # ---- 2. the constraints at z ----
    a_z, a_gz, b_z, b_gz, q_z = ood
    c = constraints_at(z, n, a_0, b_0, a_z, a_gz, b_z, b_gz)
    want_q_z = ((weights[0] * c[0] + weights[1] * c[1]) * inv((pow(z, n, P) - 1) % P) + weights[2] * c[2] + weights[3] * c[3]) % P
    if q_z != want_q_z:
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
        row, row_g = opened["trace", qi], opened["trace", (qi + B) % N]
        num = (alphas[0] * (row[0] - a_z) + alphas[1] * (row_g[0] - a_gz) + alphas[2] * (row[1] - b_z) + alphas[3] * (row_g[1] - b_gz)
               + alphas[4] * (opened["quotient", qi][0] - q_z))
        if opened["deep", qi][0] != num * inv((x_i - z) % P) % P:
            return fail("deep_value")

    # ---- 4. every fold from the opened pair (layer k lives on 7^(2^k) <w_(N / 2^k)>) ----
    last_fold = []
    for qi in qidx:
        x_i = COSET_SHIFT * pow(w_N, qi, P) % P
        prev = fold_pair(opened["deep", qi][0], opened["deep", qi + N // 2][0], betas[0], x_i)
        pos = qi
        for k in range(1, folds):
            half = (N >> k) // 2
            lo = pos % half
            if opened[f"fri{k}", pos][0] != prev:
                return fail("fri_consistency")
            x = pow(COSET_SHIFT * pow(w_N, lo, P) % P, 1 << k, P)
            prev = fold_pair(opened[f"fri{k}", lo][0], opened[f"fri{k}", lo + half][0], betas[k], x)
            pos = lo
        last_fold.append((pos, prev))

    # ---- 5. the final layer: B equal values under the last commitment, and what the last fold gave ----
    if any(v != final[0] for v in final):
        return fail("final_not_constant")
    if merkle_root_of(final) != commitments[-1]:
        return fail("final_commitment")
    if any(final[pos] != prev for pos, prev in last_fold):
        return fail("final_value")
    return True
