// Steps the proof-of-work bodies (toyni_amd/csrc/pow_kernels.hpp; include/toyni_hip.h 3n) on the CPU: the TOYNI_HD functions the three
// kernels of a grind chain run.  TEST INFRASTRUCTURE (tests/test_emu_pow.py builds it under AddressSanitizer + UBSan and judges every
// line it prints against hashlib).  The transcript and every byte string live in heap blocks of exactly their size, so a byte read or
// written past any of them ends the run.
//
// Commands on stdin, one per line; answers on stdout:
//   init <hex|->                 state = these bytes, status 0; the rest of the array is filled with A5 (stale bytes must not matter)
//   status <v>                   set the status word
//   state                        -> T <len> <status> <hex of all 1008 bytes>
//   mid                          -> M <blocks> h0 .. h7            pow_midstate (the state words after the full blocks)
//   digest <nonce>               -> D <1|2> <hex digest>           pow_candidate_state in the form the length asks for
//   accept <h0> <bits>           -> A <0|1>                        pow_accept
//   check <nonce> <bits>         -> C <0|1>                        pow_check_bytes on a heap copy of exactly len bytes
//   arm                          -> N <nonce word>                 pow_arm
//   nonce <v>                    set the nonce word
//   finish <bits> <top>          -> N <nonce word>                 pow_finish
//   search <bits> <start> <tries>  -> N <nonce word>               arm, pow_search as thread 0 of 1 (the serial search), finish
//   grid <bits> <log_tries>      -> G <workgroups>                 pow_grid_blocks
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "pow_kernels.hpp"

using namespace toyni;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}

template <bool TWO>
static Digest candidate_digest(const TranscriptState& tr, uint64_t nonce) {
    const Sha256State mid = pow_midstate(tr, tr.len);
    const PowTail<TWO> tail = pow_tail<TWO>(tr, tr.len);
    return digest_of(pow_candidate_state<TWO>(mid, tail, tr.len & 63u, nonce));
}
template <bool TWO>
static void serial_search(const TranscriptState& tr, uint32_t bits, uint64_t start, uint64_t tries, uint64_t* best) {
    const Sha256State mid = pow_midstate(tr, tr.len);
    const PowTail<TWO> tail = pow_tail<TWO>(tr, tr.len);
    pow_search<TWO>(mid, tail, tr.len & 63u, bits, start, tries, 0u, 1u, best);
}

int main() {
    TranscriptState* tr = static_cast<TranscriptState*>(aligned_alloc(16, sizeof(TranscriptState)));
    memset(tr, 0, sizeof *tr);
    std::unique_ptr<uint64_t> nonce(new uint64_t(0x1111111111111111ull));
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "init") {
            std::string hex;
            in >> hex;
            const std::vector<uint8_t> b = unhex(hex);
            if (b.size() > TRANSCRIPT_CAPACITY) return 2;
            memset(tr, 0, 16);
            memset(tr->bytes, 0xA5, TRANSCRIPT_CAPACITY);
            if (!b.empty()) memcpy(tr->bytes, b.data(), b.size());
            tr->len = (uint32_t)b.size();
        } else if (cmd == "status") {
            in >> tr->status;
        } else if (cmd == "state") {
            printf("T %u %u ", tr->len, tr->status);
            for (uint32_t k = 0; k < TRANSCRIPT_CAPACITY; ++k) printf("%02x", tr->bytes[k]);
            printf("\n");
        } else if (cmd == "mid") {
            const Sha256State m = pow_midstate(*tr, tr->len);
            printf("M %u", tr->len / 64u);
            for (int k = 0; k < 8; ++k) printf(" %u", m.h[k]);
            printf("\n");
        } else if (cmd == "digest") {
            unsigned long long v = 0;
            in >> v;
            if (!pow_fits(tr->len)) return 2;
            const bool two = pow_two_blocks(tr->len);
            const Digest d = two ? candidate_digest<true>(*tr, v) : candidate_digest<false>(*tr, v);
            printf("D %d ", two ? 2 : 1);
            for (int k = 0; k < 8; ++k)
                for (int b = 0; b < 4; ++b) printf("%02x", (d.m[k] >> (8 * b)) & 0xFFu);
            printf("\n");
        } else if (cmd == "accept") {
            unsigned long long h0 = 0;
            uint32_t bits = 0;
            in >> h0 >> bits;
            printf("A %d\n", pow_accept((uint32_t)h0, bits) ? 1 : 0);
        } else if (cmd == "check") {
            unsigned long long v = 0;
            uint32_t bits = 0;
            in >> v >> bits;
            std::unique_ptr<uint8_t[]> copy(new uint8_t[tr->len ? tr->len : 1]);
            memcpy(copy.get(), tr->bytes, tr->len);
            printf("C %d\n", pow_check_bytes(tr->len ? copy.get() : nullptr, tr->len, v, bits) ? 1 : 0);
        } else if (cmd == "arm") {
            pow_arm(*tr, nonce.get());
            printf("N %llu\n", (unsigned long long)*nonce);
        } else if (cmd == "nonce") {
            unsigned long long v = 0;
            in >> v;
            *nonce = v;
        } else if (cmd == "finish") {
            uint32_t bits = 0, top = 0;
            in >> bits >> top;
            pow_finish(*tr, nonce.get(), bits, top != 0u);
            printf("N %llu\n", (unsigned long long)*nonce);
        } else if (cmd == "search") {
            uint32_t bits = 0;
            unsigned long long start = 0, tries = 0;
            in >> bits >> start >> tries;
            pow_arm(*tr, nonce.get());
            if (tr->status == 0u) {                                // (the search kernel returns at once when the status is set)
                if (pow_two_blocks(tr->len)) serial_search<true>(*tr, bits, start, tries, nonce.get());
                else serial_search<false>(*tr, bits, start, tries, nonce.get());
            }
            pow_finish(*tr, nonce.get(), bits, start + (tries - 1u) == ~0ull);
            printf("N %llu\n", (unsigned long long)*nonce);
        } else if (cmd == "grid") {
            uint32_t bits = 0, log_tries = 0;
            in >> bits >> log_tries;
            printf("G %u\n", pow_grid_blocks(bits, log_tries));
        } else {
            fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
    }
    free(tr);
    printf("DONE\n");
    return 0;
}
