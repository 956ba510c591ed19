// Steps the device transcript (toyni_amd/csrc/transcript_kernels.hpp; include/toyni_hip.h 3l) on the CPU: the TOYNI_HD functions the
// one-wave kernels run (the argument `wave` takes the lane-spread form of absorb, as lane 0 of a one-lane wave).  TEST INFRASTRUCTURE (tests/test_emu_transcript.py builds it under
// AddressSanitizer + UBSan and judges every line it prints against hashlib; tests/test_field_contracts_transcript.py rebuilds it with
// tests/emu/field_contracts.hpp in front).  The state, every source and every output live in heap blocks of exactly their size, so a
// byte read or written past any of them ends the run.
//
// Commands on stdin, one per line; answers on stdout:
//   init <hex|->             state = these bytes, status 0; the rest of the array is filled with A5 (stale bytes must not matter)
//   status <v>               set the status word
//   absorb <hex|->           transcript_absorb
//   squeeze <count>          -> S v0 v1 ...
//   indices <count> <max>    -> I v0 v1 ...
//   state                    -> T <len> <status> <hex of all 1008 bytes>
//   reduce <u64>             -> R <residue>
//   positions <m0> <final> <idx> ...   -> P p0 p1 ...      (count = the number of indices)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "transcript_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}

int main(int argc, char** argv) {
    const bool wave = argc > 1 && !strcmp(argv[1], "wave");   // absorb through the wave form (as lane 0 of a one-lane wave)
    TranscriptState* tr = static_cast<TranscriptState*>(aligned_alloc(16, sizeof(TranscriptState)));
    memset(tr, 0, sizeof *tr);
    std::string line;
    unsigned long lineno = 0;
    while (std::getline(std::cin, line)) {
        ++lineno;
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        TOYNI_CONTRACT_TAG("emu_transcript line %lu: %s", lineno, cmd.c_str());
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
        } else if (cmd == "absorb") {
            std::string hex;
            in >> hex;
            const std::vector<uint8_t> b = unhex(hex);
            std::unique_ptr<uint8_t[]> src(new uint8_t[b.size() ? b.size() : 1]);
            if (!b.empty()) memcpy(src.get(), b.data(), b.size());
            if (wave) transcript_absorb_wave(*tr, src.get(), (uint32_t)b.size(), 0u, 1u);
            else transcript_absorb(*tr, src.get(), (uint32_t)b.size());
        } else if (cmd == "squeeze") {
            uint32_t count = 0;
            in >> count;
            std::unique_ptr<uint32_t[]> out(new uint32_t[count ? count : 1]);
            for (uint32_t k = 0; k < count; ++k) out[k] = 0xDEADBEEFu;
            transcript_squeeze(*tr, out.get(), count);
            printf("S");
            for (uint32_t k = 0; k < count; ++k) printf(" %u", out[k]);
            printf("\n");
        } else if (cmd == "indices") {
            uint32_t count = 0, max = 0;
            in >> count >> max;
            std::unique_ptr<uint32_t[]> out(new uint32_t[count]), seen(new uint32_t[count]);
            for (uint32_t k = 0; k < count; ++k) out[k] = seen[k] = 0xDEADBEEFu;
            transcript_squeeze_indices(*tr, count, max, out.get(), seen.get(), 0u, 1u, [](bool hit) { return hit; });
            printf("I");
            for (uint32_t k = 0; k < count; ++k) printf(" %u", out[k]);
            printf("\n");
        } else if (cmd == "state") {
            printf("T %u %u ", tr->len, tr->status);
            for (uint32_t k = 0; k < TRANSCRIPT_CAPACITY; ++k) printf("%02x", tr->bytes[k]);
            printf("\n");
        } else if (cmd == "reduce") {
            unsigned long long x = 0;
            in >> x;
            printf("R %u\n", bb_reduce_u64((uint64_t)x));
        } else if (cmd == "positions") {
            unsigned long long m0 = 0, fin = 0, v;
            in >> m0 >> fin;
            std::vector<uint32_t> idx;
            while (in >> v) idx.push_back((uint32_t)v);
            std::unique_ptr<uint32_t[]> src(new uint32_t[idx.size()]);
            memcpy(src.get(), idx.data(), idx.size() * sizeof(uint32_t));
            unsigned rounds = 0;
            for (unsigned long long m = m0; m > fin; m >>= 1) ++rounds;
            const uint64_t total = (uint64_t)rounds * 2u * idx.size();
            printf("P");
            for (uint64_t t = 0; t < total; ++t) printf(" %u", fri_query_position(src.get(), (uint32_t)idx.size(), m0, t));
            printf("\n");
        } else {
            fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 2;
        }
    }
    free(tr);
    printf("DONE\n");
    return 0;
}
