// Proof of work ("grinding") on the device transcript (include/toyni_hip.h 3n): between the last absorbed root and the query indices
// the prover looks for a 64-bit nonce whose hash with the transcript's state has `bits` leading zero bits, and absorbs it.
//
// The protocol is this library's own (the reference has no grinding); for a state S of `len` bytes:
//   accept(S, nonce, bits)   the first `bits` bits of SHA256(S || LE64(nonce)) are zero, the most significant bit of digest byte 0
//                            first; 0 <= bits <= 32, bits = 0 accepts everything
//   grind(S, bits, start, log_tries)   the SMALLEST nonce of [start, start + 2^log_tries) that is accepted
//   then the transcript absorbs the 8 bytes LE64(nonce) (transcript_absorb, unchanged).
// The opposite shape of everything else the transcript does: 2^bits INDEPENDENT compressions, no memory traffic.  What the candidates
// of a launch share is hashed once: the floor(len / 64) full blocks of S (the MIDSTATE, once per workgroup, by one lane, handed over
// through LDS) and the message words of the tail that hold no nonce byte (the TAIL TEMPLATE, a few uniform loads per thread).  A
// candidate then costs ONE compression when len mod 64 + 8 + 9 <= 64 and two otherwise: a template parameter, not a branch.
// Plain C++ so tests/emu can step it and tests/sim can run the search kernel's own text.
#pragma once
#include "transcript_kernels.hpp"

namespace toyni {

constexpr uint32_t POW_MAX_BITS = 32, POW_MAX_LOG_TRIES = 40;
constexpr uint64_t POW_NONE = ~(uint64_t)0;               // what the first launch of a chain arms *d_nonce with: "no hit yet"

// ---- the two atomic operations of the search, on the one word the launches of a chain share ----
// Device: agent scope -- the word is written by workgroups on other XCDs, whose L2 a plain load need not look into.  Relaxed: nothing
// else is published through it.  Host (tests/emu, tests/sim, the host pass of the product build): the compiler's own builtins.
TOYNI_HD uint64_t pow_atomic_load(const uint64_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}
TOYNI_HD void pow_atomic_min(uint64_t* p, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    uint64_t seen = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < seen && !__atomic_compare_exchange_n(p, &seen, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
#endif
}

// ---- acceptance ----
// h0 = the first state word of the digest = digest bytes 0..3 as a big-endian word: its top bit is the first bit counted
TOYNI_HD bool pow_accept(uint32_t h0, uint32_t bits) { return bits == 0u || (h0 >> (32u - bits)) == 0u; }

// ---- when a thread stops ----
// `candidate` is the nonce the thread would test next, `best` a value it has read from the shared word at some earlier time.  The
// word only ever decreases and every value stored in it is an accepted nonce, so best >= the final minimum whenever it was read: a
// thread that stops here owns no candidate below the final minimum that it has not tested.  That makes the minimum exact with no
// wait and no co-residency; a stale `best` only delays the exit.  (The classic wrong rule -- stop as soon as anything is found,
// best != POW_NONE -- returns whichever hit landed first.)  A sim driver may replace the rule: tests/sim/sim_pow.cpp shows that the
// wrong one is caught.
#ifndef TOYNI_POW_STOP_RULE
#define TOYNI_POW_STOP_RULE(candidate, best) ((candidate) > (best))
#endif
TOYNI_HD bool pow_stop(uint64_t candidate, uint64_t best) { return TOYNI_POW_STOP_RULE(candidate, best); }

// May a nonce join a state of `len`?  (transcript_fits for the 8 bytes of the absorb that ends a chain)
TOYNI_HD bool pow_fits(uint32_t len) { return transcript_fits(len, 8u); }
// does a candidate's tail (len mod 64 data bytes, 8 nonce bytes, the padding byte, the 8 length bytes) need a second block?
TOYNI_HD bool pow_two_blocks(uint32_t len) { return (len & 63u) + 8u + 9u > 64u; }

// ---- midstate: the full blocks of the state, hashed once ----
TOYNI_HD Sha256State pow_midstate(const TranscriptState& tr, uint32_t len) {
    Sha256State st = sha256_init();
    for (uint32_t b = 0; b < len / 64u; ++b) {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = sha_bswap(transcript_word(tr, 16u * b + (uint32_t)k));
        sha256_compress(st, w);
    }
    return st;
}

// ---- tail template: message word j (big-endian, counted from the start of the message) of S || 00 x 8 || 80 || 00 .. ----
// data below `len` (stale bytes of a longer, earlier state masked off), zeros where the nonce goes, the padding byte at len + 8;
// the length words are pow_tail's.  Only words that hold data are read.
TOYNI_HD uint32_t pow_tail_word(const TranscriptState& tr, uint32_t len, uint32_t j) {
    const uint32_t at = 4u * j, pad = len + 8u;
    uint32_t w = 0u;
    if (at < len) {
        w = sha_bswap(transcript_word(tr, j));
        if (len - at < 4u) w &= ~(0xFFFFFFFFu >> (8u * (len - at)));
    }
    if (pad >= at && pad < at + 4u) w |= 0x80000000u >> (8u * (pad - at));
    return w;
}
template <bool TWO>
struct PowTail { uint32_t w[TWO ? 32 : 16]; };
template <bool TWO>
TOYNI_HD PowTail<TWO> pow_tail(const TranscriptState& tr, uint32_t len) {
    constexpr int N = TWO ? 32 : 16;
    PowTail<TWO> t;
#pragma unroll
    for (int k = 0; k < N - 1; ++k) t.w[k] = pow_tail_word(tr, len, 16u * (len / 64u) + (uint32_t)k);
    t.w[N - 1] = 8u * (len + 8u);                                  // <= 8064 bits: the high length word stays the zero it is
    return t;
}

// ---- one candidate ----
// LE64(nonce) lies at byte r = len mod 64 of the tail: as big-endian words hi = n0 n1 n2 n3, lo = n4 n5 n6 n7, shifted right by
// s = r mod 4 bytes from word r / 4 on -- two words when s = 0, three otherwise.  Every register index below is a constant; which
// words take a piece is decided by comparisons with a value that is the same in every lane (r is a launch constant).
template <bool TWO>
TOYNI_HD Sha256State pow_candidate_state(const Sha256State& mid, const PowTail<TWO>& tail, uint32_t r, uint64_t nonce) {
    const uint32_t j = r >> 2, s8 = 8u * (r & 3u);
    const uint32_t hi = sha_bswap((uint32_t)nonce), lo = sha_bswap((uint32_t)(nonce >> 32));
    const uint32_t p0 = hi >> s8, p1 = s8 ? (hi << (32u - s8)) | (lo >> s8) : lo, p2 = s8 ? lo << (32u - s8) : 0u;
    Sha256State st = mid;
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t K = (uint32_t)k;
        w[k] = tail.w[k] | (K == j ? p0 : 0u) | (K == j + 1u ? p1 : 0u) | (K == j + 2u ? p2 : 0u);
    }
    sha256_compress(st, w);
    if (TWO) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t K = 16u + (uint32_t)k;
            w[k] = tail.w[TWO ? 16 + k : k] | (K == j ? p0 : 0u) | (K == j + 1u ? p1 : 0u) | (K == j + 2u ? p2 : 0u);
        }
        sha256_compress(st, w);
    }
    return st;
}

// ---- the search: what thread t of T runs (tests/emu: t = 0, T = 1 is the serial search) ----
// Tests start + t, start + t + T, ... below start + tries (tries <= 2^40; start + tries <= 2^64, so start + off never wraps).  The
// shared word is read one candidate AHEAD -- the load is in flight across the compression -- which the stop rule allows: any value
// ever read from the word is at least the final minimum.
// A hit is published INSIDE the iteration that finds it, and the thread leaves through the stop rule of the next one (its next
// candidate exceeds its own hit).  Leaving from the hit itself reads the same, but lets the compiler move the atomic behind the loop,
// where a wave executes it only after its LAST lane has left: the other 63 lanes would search on without seeing their neighbour's hit.
template <bool TWO>
TOYNI_HD void pow_search(const Sha256State& mid, const PowTail<TWO>& tail, uint32_t r, uint32_t bits, uint64_t start, uint64_t tries, uint64_t t,
                         uint64_t T, uint64_t* best) {
    uint64_t seen = pow_atomic_load(best);
    for (uint64_t off = t; off < tries; off += T) {
        const uint64_t candidate = start + off;
        if (pow_stop(candidate, seen)) return;
        seen = pow_atomic_load(best);
        if (pow_accept(pow_candidate_state<TWO>(mid, tail, r, candidate).h[0], bits)) {
            pow_atomic_min(best, candidate);
            if (candidate < seen) seen = candidate;
        }
    }
}

// ---- accept() on plain bytes: the verifier's one hash (toyni_pow_check_host), any length ----
TOYNI_HD bool pow_check_bytes(const uint8_t* state, uint64_t len, uint64_t nonce, uint32_t bits) {
    Sha256State st = sha256_init();
    uint32_t w[16];
    const uint64_t full = len / 64u;
    for (uint64_t b = 0; b < full; ++b) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint8_t* p = state + 64u * b + 4u * (uint64_t)k;
            w[k] = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
        }
        sha256_compress(st, w);
    }
    const uint32_t r = (uint32_t)(len & 63u), used = r + 8u;       // bytes of the tail in front of the padding byte
    const uint32_t nblocks = used + 9u > 64u ? 2u : 1u;
    const uint64_t nbits = 8u * (len + 8u);
    for (uint32_t b = 0; b < nblocks; ++b) {
        for (uint32_t k = 0; k < 16u; ++k) {
            uint32_t word = 0u;
            for (uint32_t i = 0; i < 4u; ++i) {
                const uint32_t at = 64u * b + 4u * k + i;
                const uint32_t byte = at < r ? state[64u * full + at] : at < used ? (uint32_t)(nonce >> (8u * (at - r))) & 0xFFu : at == used ? 0x80u : 0u;
                word = word << 8 | byte;
            }
            w[k] = word;
        }
        if (b == nblocks - 1u) { w[14] = (uint32_t)(nbits >> 32); w[15] = (uint32_t)nbits; }
        sha256_compress(st, w);
    }
    return pow_accept(st.h[0], bits);
}

// ---- the grid of the search ----
// Workgroups of POW_T threads.  A hit is expected after 2^bits candidates, so more than a few times 2^bits threads only hash
// candidates that cannot win: 4 x 2^bits threads (the first row of the grid then holds no hit with probability e^-4), no more than the
// window, and no more than 3 workgroups per CU -- 768: the search kernel's registers admit three waves per SIMD (tests/
// test_pow_resources.py holds the build to that), so the whole grid is resident at once and no workgroup starts its walk late.  At most
// 256 workgroups or a multiple of 256.  The RESULT does not depend on it.
constexpr uint32_t POW_T = 256, POW_MAX_BLOCKS = 768;
TOYNI_HD uint32_t pow_grid_blocks(uint32_t bits, uint32_t log_tries) {
    const uint32_t log_threads = bits + 2u < log_tries ? bits + 2u : log_tries;
    if (log_threads <= 8u) return 1u;
    return log_threads - 8u >= 10u ? POW_MAX_BLOCKS : 1u << (log_threads - 8u);
}

// ---- the two ends of a chain, one thread each ----
// First launch: a transcript whose status is set, or that cannot take the 8 bytes (refused into `status` here, before the search),
// gives *nonce = 0 and nothing else happens in the chain; otherwise the word is armed.
TOYNI_HD void pow_arm(TranscriptState& tr, uint64_t* nonce) {
    uint32_t status = tr.status;
    if (status == 0u && !pow_fits(tr.len)) tr.status = status = TRANSCRIPT_E_RANGE;
    *nonce = status ? 0u : POW_NONE;
}
// Last launch: "no hit" becomes the failure status (the transcript otherwise unchanged, *nonce = 0); a hit is absorbed.  A window that
// reaches 2^64 - 1 (`top`) owns the one candidate whose value IS the armed word: it is tested here.
TOYNI_HD void pow_finish(TranscriptState& tr, uint64_t* nonce, uint32_t bits, bool top) {
    if (tr.status != 0u) { *nonce = 0u; return; }
    const uint64_t v = *nonce;
    if (v == POW_NONE && !(top && pow_check_bytes(tr.bytes, tr.len, v, bits))) {
        tr.status = TRANSCRIPT_E_RANGE;
        *nonce = 0u;
        return;
    }
    uint8_t le[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) le[i] = (uint8_t)(v >> (8 * i));
    transcript_absorb(tr, le, 8u);
}

}  // namespace toyni
