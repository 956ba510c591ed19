// Verification of a batch of Fibonacci proofs on the device (include/toyni_hip.h 3t).
//
// What it reproduces: StarkVerifier::verify (src/verifier.rs:14-232) over a proof laid out as a fixed-size byte image
// (toyni_fib_proof_layout of the header).  The verifier derives everything it can itself -- the transcript from "toyni-stark-v1", z,
// the betas, the query indices and every position a query opens -- and reads from the image only what the prover claims: roots,
// out-of-domain values, claimed indices, the final layer and the opening records (the record of toyni_merkle_open_device:
// depth x 32 path bytes | 16 salt bytes | the value as 8 LE bytes | depth position bytes | zero padding to 8).
// ONE deliberate strictness over the reference: a record counts only if its position bytes spell the index the verifier derived
// (byte l = bit l of the index); the reference trusts the prover's flags for the FRI openings.
// Nothing derived from the image is ever used as an address: indices and positions are compared, never dereferenced, and the one
// index into the final layer is a derived index reduced below final_size.
// The bodies are plain C++ so that the CPU drivers can step them; they reuse sha256_compress / merkle_leaf / merkle_node, the
// transcript bodies, transcript_squeeze_point and the field primitives as they are.
#pragma once
#include "prover_kernels.hpp"
#include "transcript_kernels.hpp"
#include "fib_dz_kernels.hpp"

namespace toyni {

constexpr uint32_t VERIFY_WAVE = 64;                // the one-wave kernels' block
constexpr uint32_t VERIFY_MAX_GROUPS = 32;          // groups per launch of the record kernel, as toyni_merkle_open_groups_device
constexpr uint32_t FIBV_QUERIES = 44;               // NUM_QUERIES, src/fibonacci.rs:11
constexpr uint32_t FIBV_LOG_BLOWUP = 5, FIBV_SHIFT = 7, FIBV_MASK_DEGREE = 3 * FIBV_QUERIES + 8;
constexpr uint32_t FIBV_MAX_FINAL = 16;             // final_size = N / next_pow2(n + MASK_DEGREE) <= 16 with blow-up 32

// the verdict codes, in the order in which src/verifier.rs visits its checks
constexpr uint32_t FIBV_ACCEPT = 0, FIBV_MALFORMED = 1, FIBV_OOD = 2, FIBV_FINAL_NOT_CONSTANT = 3, FIBV_FINAL_COMMITMENT = 4, FIBV_QUERY_INDEX = 5,
                   FIBV_TRACE_MERKLE = 6, FIBV_QUOTIENT_MERKLE = 7, FIBV_DEEP_MERKLE = 8, FIBV_DEEP_VALUE = 9, FIBV_FRI_FIRST = 16, FIBV_FINAL_VALUE = 255;
TOYNI_HD uint32_t fibv_fri_merkle(uint32_t k) { return FIBV_FRI_FIRST + 2u * (k - 1u); }        // layer k = 1 .. folds - 1
TOYNI_HD uint32_t fibv_fri_consistency(uint32_t k) { return FIBV_FRI_FIRST + 1u + 2u * (k - 1u); }
TOYNI_HD uint32_t fibv_key(uint32_t query_plus_1, uint32_t code) { return (query_plus_1 << 8) | code; }

// ---- one opening record ----
struct alignas(8) VerifyPair { uint32_t x, y; };    // records are 8-byte aligned: every load of a record is one of these
TOYNI_HD uint32_t verify_record_bytes(uint32_t depth) { return 32u * depth + 24u + ((depth + 7u) & ~7u); }
TOYNI_HD bool verify_canonical(const VerifyPair& v) { return v.y == 0u && v.x < BB_P; }   // what a BabyBear can hold
TOYNI_HD VerifyPair verify_record_value(const uint8_t* rec, uint32_t depth) { return reinterpret_cast<const VerifyPair*>(rec)[4u * depth + 2u]; }

// 1: the record's leaf and path hash to `root` (8 memory words), its value is canonical and its position bytes spell `index`.
// In a tree whose leaf count is no power of two an odd level pairs its last node with itself, and MerkleTree::get_proof
// (src/merkle.rs:50-80) writes position 1 there: that byte is expected at such a level, whatever the index's bit.
TOYNI_HD uint32_t merkle_verify_record(const uint8_t* rec, uint32_t depth, uint64_t leaves, bool salted, uint32_t index, const uint32_t* root) {
    const VerifyPair* p = reinterpret_cast<const VerifyPair*>(rec);
    const VerifyPair s0 = p[4u * depth], s1 = p[4u * depth + 1u], v = p[4u * depth + 2u];
    const uint8_t* pos = rec + 32u * depth + 24u;
    bool ok = verify_canonical(v) && index < leaves;
    uint64_t m = leaves;                              // nodes of level l
    const uint32_t salt[4] = {s0.x, s0.y, s1.x, s1.y};
    Digest cur = merkle_leaf(v.x, salted ? salt : nullptr);
    for (uint32_t l = 0; l < depth; ++l) {
        const VerifyPair a = p[4u * l], b = p[4u * l + 1u], c = p[4u * l + 2u], d = p[4u * l + 3u];
        const Digest sib{{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y}};
        const uint32_t cur_at = index >> l;
        const uint32_t bit = cur_at & 1u;             // 1: this node is the right input, the sibling the left
        ok = ok && (uint32_t)pos[l] == (bit | ((uint64_t)cur_at + 1u >= m ? 1u : 0u));
        m = (m + 1u) >> 1;
        Digest left, right;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            left.m[j] = bit ? sib.m[j] : cur.m[j];
            right.m[j] = bit ? cur.m[j] : sib.m[j];
        }
        cur = merkle_node(left, right);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) ok = ok && cur.m[j] == root[j];
    return ok ? 1u : 0u;
}

// The groups of one launch.  Record r of group g of proof b lies at records[g] + b * record_stride[g] + r * verify_record_bytes(depth[g]),
// its expected index at indices[g][b * index_stride[g] + r], its root at root[g] + b * root_stride[g], and its word goes to
// flags[g][b * flag_stride[g] + r].  first[g] = the records of the groups before g.
struct MerkleVerifyGroups {
    uint32_t ngroups, batch;
    uint64_t first[VERIFY_MAX_GROUPS + 1];
    const uint8_t* records[VERIFY_MAX_GROUPS];
    uint64_t record_stride[VERIFY_MAX_GROUPS];     // bytes
    const uint32_t* indices[VERIFY_MAX_GROUPS];
    uint64_t index_stride[VERIFY_MAX_GROUPS];      // words
    const uint8_t* root[VERIFY_MAX_GROUPS];
    uint64_t root_stride[VERIFY_MAX_GROUPS];       // bytes
    uint32_t* flags[VERIFY_MAX_GROUPS];
    uint64_t flag_stride[VERIFY_MAX_GROUPS];       // words
    uint64_t leaves[VERIFY_MAX_GROUPS];
    uint32_t depth[VERIFY_MAX_GROUPS], salted[VERIFY_MAX_GROUPS];
};
// item t of first[ngroups] x batch, the proof index fastest: a wave walks paths of one depth once the batch reaches 64
TOYNI_HD void merkle_verify_item(const MerkleVerifyGroups& a, uint64_t t) {
    const uint64_t rid = t / a.batch, b = t % a.batch;
    uint32_t g = 0;
    while (g + 1u < a.ngroups && rid >= a.first[g + 1u]) ++g;
    const uint64_t r = rid - a.first[g];
    const uint32_t depth = a.depth[g];
    const uint8_t* rec = a.records[g] + b * a.record_stride[g] + r * verify_record_bytes(depth);
    const uint32_t index = a.indices[g][b * a.index_stride[g] + r];
    a.flags[g][b * a.flag_stride[g] + r] =
        merkle_verify_record(rec, depth, a.leaves[g], a.salted[g] != 0u, index, reinterpret_cast<const uint32_t*>(a.root[g] + b * a.root_stride[g]));
}

// ---- the composite call: shape of an image and of a proof's part of the work buffer ----
// Work buffer of proof b, in words from b * work_stride: the transcript (256 words), z, the key of the global checks, the betas, the
// derived indices, the keys of the 44 queries, the expected index of every record, the word of every record.
constexpr uint32_t FIBV_W_Z = 256, FIBV_W_GLOBAL = 257, FIBV_W_BETAS = 260, FIBV_W_INDICES = 292, FIBV_W_QKEYS = 336, FIBV_W_POS = 380;
constexpr uint32_t FIBV_MAX_FOLDS = FIBV_W_INDICES - FIBV_W_BETAS;   // 32 betas
struct FibVerifyArgs {
    uint32_t log_n, log_N, folds, final_size;
    uint32_t ood_word, index_word, final_word;     // word offsets in an image
    uint32_t nrecords;                             // 44 (4 + 2 folds)
    uint64_t image_stride;                         // bytes
    uint64_t work_stride;                          // words
    uint32_t b1R, b2R;                             // FibCheckArgs: Montgomery forms of g^(n-1), g^(n-2)
    uint32_t shift_invR, wNR;                      // Montgomery forms of 7^-1 and of the root of order N
    uint32_t ngroups;                              // folds + 2: trace, quotient, layer 0 (DEEP), layers 1 .. folds - 1
    uint32_t group_first[VERIFY_MAX_GROUPS + 1];   // the records before group g
    uint32_t group_depth[VERIFY_MAX_GROUPS];
    uint64_t group_byte[VERIFY_MAX_GROUPS];        // byte offset of group g's first record in an image
};
TOYNI_HD const uint8_t* fibv_record(const FibVerifyArgs& a, const uint8_t* image, uint32_t g, uint32_t r) {
    return image + a.group_byte[g] + (uint64_t)r * verify_record_bytes(a.group_depth[g]);
}
// the low word of a record's value, reduced (a value that is not canonical is MALFORMED's business)
TOYNI_HD uint32_t fibv_value(const FibVerifyArgs& a, const uint8_t* image, uint32_t g, uint32_t r) {
    return dz_reduce(verify_record_value(fibv_record(a, image, g, r), a.group_depth[g]).x);
}

// ---- a. transcript replay: ONE thread ----
// absorb_field (src/transcript.rs): the value as 8 little-endian bytes
TOYNI_HD void fibv_absorb_field(TranscriptState& tr, uint32_t v) {
    const uint32_t len = tr.len;
    if (tr.status != 0u) return;
    if (!transcript_fits(len, 8u)) { tr.status = TRANSCRIPT_E_RANGE; return; }
    for (uint32_t j = 0; j < 4u; ++j) tr.bytes[len + j] = (uint8_t)(v >> (8u * j));
    for (uint32_t j = 4; j < 8u; ++j) tr.bytes[len + j] = 0u;
    tr.len = len + 8u;
}
// Writes the transcript, z, `folds` betas and 44 indices of one proof.  A transcript that refuses (no point within FIB_POINT_TRIES
// squeezes, no 44 distinct indices within the budget: chances of 2^-100 and less) keeps its sticky status, which the global checks
// report as MALFORMED.
TOYNI_HD void fib_verify_replay(const FibVerifyArgs& a, const uint8_t* image, uint32_t* work) {
    TranscriptState& tr = *reinterpret_cast<TranscriptState*>(work);
    const char tag[14] = {'t', 'o', 'y', 'n', 'i', '-', 's', 't', 'a', 'r', 'k', '-', 'v', '1'};
    tr.len = 14u;
    tr.status = 0u;
    tr.reserved[0] = tr.reserved[1] = 0u;
    for (uint32_t j = 0; j < 14u; ++j) tr.bytes[j] = (uint8_t)tag[j];
    const uint32_t* words = reinterpret_cast<const uint32_t*>(image);
    transcript_absorb(tr, image, 64u);                                           // the trace root, the quotient root
    transcript_squeeze_point(tr, a.log_N, a.shift_invR, FIB_POINT_TRIES, work + FIBV_W_Z);
    for (uint32_t j = 0; j < 4u; ++j) fibv_absorb_field(tr, words[a.ood_word + j]);
    transcript_absorb(tr, image + 64u, 32u);                                     // fri_commitments[0]
    for (uint32_t k = 1; k <= a.folds; ++k) {
        transcript_squeeze(tr, work + FIBV_W_BETAS + (k - 1u), 1u);
        transcript_absorb(tr, image + 32u * (2u + k), 32u);
    }
    uint32_t* idx = work + FIBV_W_INDICES;
    transcript_squeeze_indices(tr, FIBV_QUERIES, 1u << (a.log_N - 1u), idx, idx, 0u, 1u, [](bool hit) { return hit; });
}

// ---- b. the global checks and c. the positions: ONE wave ----
// expected index of record t of an image, from the derived indices: the arithmetic of toyni_query_rows_batch_device (rows qi,
// qi + 32, qi + 64 mod N), the indices themselves, and toyni_fri_query_positions_batch_device over the layers 0 .. folds - 2
TOYNI_HD uint32_t fibv_position(const FibVerifyArgs& a, const uint32_t* idx, uint32_t t) {
    const uint64_t N = (uint64_t)1 << a.log_N;
    if (t < 3u * FIBV_QUERIES) return (uint32_t)(((uint64_t)idx[t / 3u] + ((uint64_t)(t % 3u) << FIBV_LOG_BLOWUP)) % N);   // query_row, offsets 0, 32, 64
    if (t < 4u * FIBV_QUERIES) return idx[t - 3u * FIBV_QUERIES];
    return fri_query_position(idx, FIBV_QUERIES, N, t - 4u * FIBV_QUERIES);
}
// lds_tree: FIBV_MAX_FINAL digests the whole wave can read; any_lane as in transcript_squeeze_indices_kernel.  Every loop count and
// every call of any_lane / TOYNI_WAVE_ORDER below is the same in every lane.
template <class AnyLane>
TOYNI_HD void fib_verify_global(const FibVerifyArgs& a, const uint8_t* image, uint32_t* work, Digest* lds_tree, uint32_t lane, uint32_t nlanes,
                                AnyLane&& any_lane) {
    const uint32_t* words = reinterpret_cast<const uint32_t*>(image);
    const uint32_t fs = a.final_size;
    // every field word of the image is canonical
    bool bad = false;
    for (uint32_t t = lane; t < 4u + fs; t += nlanes) bad |= (t < 4u ? words[a.ood_word + t] : words[a.final_word + (t - 4u)]) >= BB_P;
    for (uint32_t t = lane; t < a.nrecords; t += nlanes) {
        uint32_t g = 0;
        while (g + 1u < a.ngroups && t >= a.group_first[g + 1u]) ++g;
        bad |= !verify_canonical(verify_record_value(fibv_record(a, image, g, t - a.group_first[g]), a.group_depth[g]));
    }
    const bool malformed = any_lane(bad);
    // the final layer is constant (src/verifier.rs:80-84) ...
    const bool not_constant = any_lane(lane < fs && words[a.final_word + lane] != words[a.final_word]);
    // ... and the unsalted tree over it has the last commitment as its root (:85-91)
    if (lane < fs) lds_tree[lane] = merkle_leaf(words[a.final_word + lane], nullptr);
    TOYNI_WAVE_ORDER();
    for (uint32_t m = fs >> 1; m >= 1u; m >>= 1) {
        Digest d{};
        if (lane < m) d = merkle_node(lds_tree[2u * lane], lds_tree[2u * lane + 1u]);
        TOYNI_WAVE_ORDER();                           // every lane has read its two children before any lane overwrites one
        if (lane < m) lds_tree[lane] = d;
        TOYNI_WAVE_ORDER();
    }
    if (lane == 0u) {
        const uint32_t* root = words + 8u * (a.folds + 2u);
        bool commitment = true;
        for (uint32_t j = 0; j < 8u; ++j) commitment = commitment && lds_tree[0].m[j] == root[j];
        // C(z) = Q(z) Z(z) (:44-49)
        FibDeepRecord rec;
        uint32_t check = 0u;
        fib_deep_prepare(work + FIBV_W_Z, words + a.ood_word, FibCheckArgs{a.b1R, a.b2R, a.log_n}, &rec, &check);
        const TranscriptState& tr = *reinterpret_cast<const TranscriptState*>(work);
        work[FIBV_W_GLOBAL] = (malformed || tr.status != 0u) ? FIBV_MALFORMED
                              : !check                       ? FIBV_OOD
                              : not_constant                 ? FIBV_FINAL_NOT_CONSTANT
                              : !commitment                  ? FIBV_FINAL_COMMITMENT
                                                             : FIBV_ACCEPT;
    }
    const uint32_t* idx = work + FIBV_W_INDICES;
    for (uint32_t t = lane; t < a.nrecords; t += nlanes) work[FIBV_W_POS + t] = fibv_position(a, idx, t);
}

// ---- e. the checks of one query (src/verifier.rs:93-229, steps 6a - 6g): the key of the first one that fails, 0 if none does ----
// one fold step: (a + b) / 2 + (a - b) / 2 * beta / x, x^-1 in Montgomery form
TOYNI_HD uint32_t fibv_fold(uint32_t va, uint32_t vb, uint32_t beta, uint32_t xinvR) {
    return bb_add(bb_halve(bb_add(va, vb)), mont_mul(mont_mul(bb_halve(bb_sub(va, vb)), to_mont(beta)), xinvR));
}
// (7 w_N^e)^(2^k) in Montgomery form
TOYNI_HD uint32_t fibv_point(const FibVerifyArgs& a, uint32_t e, uint32_t k) {
    uint32_t xR = to_mont(mont_mul(FIBV_SHIFT, mont_pow(a.wNR, e)));
    for (uint32_t i = 0; i < k; ++i) xR = mont_mul(xR, xR);
    return xR;
}
TOYNI_HD uint32_t fib_verify_query(const FibVerifyArgs& a, const uint8_t* image, const uint32_t* work, uint32_t q) {
    const uint32_t* words = reinterpret_cast<const uint32_t*>(image);
    const uint32_t* flags = work + FIBV_W_POS + a.nrecords;
    const uint32_t qi = work[FIBV_W_INDICES + q];
    uint32_t code = 0u;
    const auto fail = [&code](bool failed, uint32_t c) { if (code == 0u && failed) code = c; };
    fail(words[a.index_word + q] != qi, FIBV_QUERY_INDEX);
    fail(!(flags[a.group_first[0] + 3u * q] && flags[a.group_first[0] + 3u * q + 1u] && flags[a.group_first[0] + 3u * q + 2u]), FIBV_TRACE_MERKLE);
    fail(!flags[a.group_first[1] + q], FIBV_QUOTIENT_MERKLE);
    fail(!(flags[a.group_first[2] + 2u * q] && flags[a.group_first[2] + 2u * q + 1u]), FIBV_DEEP_MERKLE);
    // the DEEP value rebuilt from the opened trace and quotient values (:150-168)
    const uint32_t z = dz_reduce(work[FIBV_W_Z]);
    const uint32_t t_z = dz_reduce(words[a.ood_word]), t_gz = dz_reduce(words[a.ood_word + 1u]), t_ggz = dz_reduce(words[a.ood_word + 2u]),
                   q_z = dz_reduce(words[a.ood_word + 3u]);
    const uint32_t x0R = fibv_point(a, qi, 0u);
    const uint32_t ixzR = mont_inv_chain(bb_sub(x0R, to_mont(z)));
    const uint32_t sum = bb_add(bb_add(bb_sub(fibv_value(a, image, 1u, q), q_z), bb_sub(fibv_value(a, image, 0u, 3u * q + 2u), t_ggz)),
                                bb_add(bb_sub(fibv_value(a, image, 0u, 3u * q + 1u), t_gz), bb_sub(fibv_value(a, image, 0u, 3u * q), t_z)));
    const uint32_t a0 = fibv_value(a, image, 2u, 2u * q), b0 = fibv_value(a, image, 2u, 2u * q + 1u);
    fail(a0 != mont_mul(sum, ixzR), FIBV_DEEP_VALUE);
    // the fold chain (:170-224)
    uint32_t prev = fibv_fold(a0, b0, dz_reduce(work[FIBV_W_BETAS]), mont_inv_chain(x0R));
    uint32_t pos = qi;
    for (uint32_t k = 1; k < a.folds; ++k) {
        const uint32_t half = 1u << (a.log_N - k - 1u), lo = pos & (half - 1u);
        const uint32_t f = a.group_first[2u + k] + 2u * q;
        fail(!(flags[f] && flags[f + 1u]), fibv_fri_merkle(k));
        const uint32_t va = fibv_value(a, image, 2u + k, 2u * q), vb = fibv_value(a, image, 2u + k, 2u * q + 1u);
        fail((pos == lo ? va : vb) != prev, fibv_fri_consistency(k));
        prev = fibv_fold(va, vb, dz_reduce(work[FIBV_W_BETAS + k]), mont_inv_chain(fibv_point(a, lo, k)));
        pos = lo;
    }
    fail(dz_reduce(words[a.final_word + (pos & (a.final_size - 1u))]) != prev, FIBV_FINAL_VALUE);   // :226
    return code ? fibv_key(q + 1u, code) : 0u;
}

// ---- f. the verdict: the smallest key that is not zero, the global checks' first (their query field is zero) ----
TOYNI_HD uint32_t fib_verify_verdict(const uint32_t* work) {
    uint32_t best = work[FIBV_W_GLOBAL];
    if (best) return fibv_key(0u, best);
    for (uint32_t q = 0; q < FIBV_QUERIES; ++q) {
        const uint32_t k = work[FIBV_W_QKEYS + q];
        if (k && (!best || k < best)) best = k;
    }
    return best;
}

}  // namespace toyni
