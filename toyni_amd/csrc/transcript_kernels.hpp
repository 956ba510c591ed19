// The Fiat-Shamir transcript in device memory (include/toyni_hip.h 3l).
//
// What it reproduces, byte for byte: FiatShamirTranscript (src/transcript.rs) with BabyBear::from_bytes_mod_order
// (src/babybear.rs:65-71):
//   absorb(data)              state = state || data
//   squeeze_challenge()       h = SHA256(state); state = h; return (h[0..8] as a little-endian u64) mod p
//   squeeze_indices(count, max)   the same chain with the value taken mod max; a value seen before is dropped
// The reference's state is a heap Vec<u8> without a bound; here it is a fixed 1008-byte array behind its length and a sticky status
// word (TranscriptState = toyni_transcript of the header), and what the array cannot hold is refused into `status`.  After the first
// squeeze the state is always one digest, so a chain of squeezes hashes 32 bytes -- one block -- per step and carries the digest in
// registers; only the first hash of a call walks the byte array (up to 16 blocks).  Every step depends on the one before it: the
// chains are serial by definition: absorb and squeeze are written for ONE thread (a kernel runs them on one lane), and only the index
// squeeze, which searches the values seen so far with the lanes of its wave, and the byte copy of a long absorb use more.
// Plain C++ so tests/emu can step it.
#pragma once
#include "merkle_kernels.hpp"

namespace toyni {

constexpr uint32_t TRANSCRIPT_CAPACITY = 1008;
constexpr uint32_t TRANSCRIPT_E_RANGE = 10006;           // TOYNI_E_RANGE of the header: what `status` receives
constexpr uint32_t TRANSCRIPT_MAX_INDICES = 256;
struct alignas(16) TranscriptState {
    uint32_t len, status, reserved[2];
    uint8_t bytes[TRANSCRIPT_CAPACITY];
};
static_assert(sizeof(TranscriptState) == 1024, "toyni_transcript is 1024 bytes");

// bytes 4 j .. 4 j + 3 of the state as one little-endian word (the array starts 16-byte aligned: one aligned load)
TOYNI_HD uint32_t transcript_word(const TranscriptState& tr, uint32_t j) {
    uint32_t w;
    __builtin_memcpy(&w, tr.bytes + 4u * j, 4);
    return w;
}

// message word j (big-endian) of the padded message of `len` state bytes: data, then 80, then zeros; the length words are the caller's.
// Nothing at or beyond `len` is interpreted (stale bytes of a longer, earlier state are masked off), nothing beyond the last word that
// holds data is read.
TOYNI_HD uint32_t transcript_message_word(const TranscriptState& tr, uint32_t len, uint32_t j) {
    const uint32_t at = 4u * j;
    if (at + 4u <= len) return sha_bswap(transcript_word(tr, j));
    if (at > len) return 0u;
    const uint32_t r = len - at;                                   // 0 .. 3 data bytes in this word
    const uint32_t data = r ? (sha_bswap(transcript_word(tr, j)) & ~(0xFFFFFFFFu >> (8u * r))) : 0u;
    return data | (0x80000000u >> (8u * r));
}

// SHA256(state bytes 0 .. len), len <= TRANSCRIPT_CAPACITY: ceil((len + 9) / 64) blocks.  The block loop is rolled (its trip count is
// data); inside it every register index is a constant.
TOYNI_HD Digest transcript_hash_state(const TranscriptState& tr, uint32_t len) {
    const uint32_t nblocks = (len + 9u + 63u) / 64u;
    Sha256State st = sha256_init();
    for (uint32_t b = 0; b < nblocks; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = transcript_message_word(tr, len, 16u * b + (uint32_t)k);
        if (b == nblocks - 1u) w[15] = 8u * len;                   // <= 8064 bits: the high length word stays the zero it is
        sha256_compress(st, w);
    }
    return digest_of(st);
}
// SHA256 of a state that is one digest (every step of a chain but the first): 32 bytes, one block
TOYNI_HD Digest transcript_hash_digest(const Digest& d) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = sha_bswap(d.m[k]);
    w[8] = 0x80000000u;
#pragma unroll
    for (int k = 9; k < 15; ++k) w[k] = 0u;
    w[15] = 256u;
    Sha256State st = sha256_init();
    sha256_compress(st, w);
    return digest_of(st);
}
// the first 8 bytes of a digest as a little-endian u64
TOYNI_HD uint64_t transcript_value(const Digest& d) { return ((uint64_t)d.m[1] << 32) | d.m[0]; }

// state = one digest
TOYNI_HD void transcript_store_digest(TranscriptState& tr, const Digest& d) {
#pragma unroll
    for (int k = 0; k < 8; ++k) __builtin_memcpy(tr.bytes + 4 * k, &d.m[k], 4);
    tr.len = 32u;
}

// One step of a chain: the hash of the current state -- `d` when `have` (a digest carried in registers), the byte array otherwise.
struct TranscriptChain { Digest d; bool have; };
TOYNI_HD void transcript_step(const TranscriptState& tr, uint32_t len, TranscriptChain& c) {
    c.d = c.have ? transcript_hash_digest(c.d) : transcript_hash_state(tr, len);
    c.have = true;
}

// ---- absorb ----
// May `n` bytes join a state of `len`?  (len itself is checked too: a state copied in by the caller may carry any word there)
TOYNI_HD bool transcript_fits(uint32_t len, uint32_t n) { return len <= TRANSCRIPT_CAPACITY && n <= TRANSCRIPT_CAPACITY - len; }
// One thread: refused into `status`, or appended.  (What a round of the fused commit phase runs on one lane for a 32-byte root.)
TOYNI_HD void transcript_absorb(TranscriptState& tr, const uint8_t* src, uint32_t n) {
    const uint32_t len = tr.len;
    if (tr.status != 0u) return;
    if (!transcript_fits(len, n)) { tr.status = TRANSCRIPT_E_RANGE; return; }
    for (uint32_t i = 0; i < n; ++i) tr.bytes[len + i] = src[i];
    tr.len = len + n;
}
// The same with the copy spread over the lanes of one wave (an absorb may be a thousand bytes): every lane reads the two words before
// lane 0 stores either.
TOYNI_HD void transcript_absorb_wave(TranscriptState& tr, const uint8_t* src, uint32_t n, uint32_t lane, uint32_t nlanes) {
    const uint32_t len = tr.len, status = tr.status;
    TOYNI_WAVE_ORDER();
    if (status != 0u) return;
    if (!transcript_fits(len, n)) {
        if (lane == 0u) tr.status = TRANSCRIPT_E_RANGE;
        return;
    }
    for (uint32_t i = lane; i < n; i += nlanes) tr.bytes[len + i] = src[i];
    if (lane == 0u) tr.len = len + n;
}

// ---- squeeze ----
// One thread: out[k] = the k-th challenge, k < count; a transcript whose status is set stays as it is and gives zeros.
TOYNI_HD void transcript_squeeze(TranscriptState& tr, uint32_t* out, uint32_t count) {
    const uint32_t len = tr.len, status = tr.status;
    if (status != 0u || len > TRANSCRIPT_CAPACITY) {
        for (uint32_t k = 0; k < count; ++k) out[k] = 0u;
        if (status == 0u) tr.status = TRANSCRIPT_E_RANGE;
        return;
    }
    if (count == 0u) return;
    TranscriptChain c{Digest{}, false};
    for (uint32_t k = 0; k < count; ++k) {
        transcript_step(tr, len, c);
        out[k] = bb_reduce_u64(transcript_value(c.d));
    }
    transcript_store_digest(tr, c.d);
}

// ---- squeeze_indices ----
// Is `idx` among seen[0 .. found)?  This lane's share of the list; the caller joins the lanes' answers.
TOYNI_HD bool transcript_seen(const uint32_t* seen, uint32_t found, uint32_t idx, uint32_t lane, uint32_t nlanes) {
    bool hit = false;
    for (uint32_t j = lane; j < found; j += nlanes) hit |= seen[j] == idx;
    return hit;
}
// count <= TRANSCRIPT_MAX_INDICES distinct values below `max` in order of first appearance.  `seen`: count words that the whole wave
// can read (LDS); any_lane(bool) = true where the flag is set in some lane.  The loop runs at most 64 count + 64 hashes -- with
// count <= max the chance of needing more is nil, the bound is what keeps ANY input from spinning -- and then refuses into `status`.
// Every lane computes the same hashes, so every loop count here is the same in every lane.
template <class AnyLane>
TOYNI_HD void transcript_squeeze_indices(TranscriptState& tr, uint32_t count, uint32_t max, uint32_t* out, uint32_t* seen, uint32_t lane,
                                         uint32_t nlanes, AnyLane&& any_lane) {
    const uint32_t len = tr.len, status = tr.status;
    bool ok = status == 0u && len <= TRANSCRIPT_CAPACITY;
    TranscriptChain c{Digest{}, false};
    uint32_t found = 0;
    if (ok) {
        const uint32_t budget = 64u * count + 64u;
        for (uint32_t h = 0; h < budget && found < count; ++h) {
            transcript_step(tr, len, c);
            const uint32_t idx = (uint32_t)(transcript_value(c.d) % max);
            if (!any_lane(transcript_seen(seen, found, idx, lane, nlanes))) {
                if (lane == 0u) seen[found] = idx;
                TOYNI_WAVE_ORDER();                                 // the wave's own store, read back by its other lanes in program order
                ++found;
            }
        }
        ok = found == count;
    }
    if (!ok) {
        for (uint32_t k = lane; k < count; k += nlanes) out[k] = 0u;
        TOYNI_WAVE_ORDER();
        if (status == 0u && lane == 0u) tr.status = TRANSCRIPT_E_RANGE;
        return;
    }
    for (uint32_t k = lane; k < count; k += nlanes) out[k] = seen[k];
    TOYNI_WAVE_ORDER();                                             // every lane has read and hashed the old state before lane 0 replaces it
    if (lane == 0u) transcript_store_digest(tr, c.d);
}

// ---- the positions a query opens in every layer but the last (src/fibonacci.rs:268-283) ----
// item t of rounds x 2 count: layer k = t / (2 count) of size m0 >> k, query q = (t / 2) mod count, the index itself or its pair
TOYNI_HD uint32_t fri_query_position(const uint32_t* indices, uint32_t count, uint64_t m0, uint64_t t) {
    const uint64_t k = t / (2u * (uint64_t)count), j = t % (2u * (uint64_t)count);
    const uint64_t half = (m0 >> k) >> 1;
    return (uint32_t)((indices[j >> 1] & (half - 1u)) + ((j & 1u) ? half : 0u));
}

// ---- the record a round of the commit phase leaves for the next fold ----
// beta (plain canonical) times a host constant cR2 = c R^2 mod p  ->  the Montgomery form of beta c
TOYNI_HD uint32_t transcript_factor(uint32_t beta, uint32_t cR2) { return mont_mul(beta, cR2); }

}  // namespace toyni
