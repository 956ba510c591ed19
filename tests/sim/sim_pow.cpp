// Runs the three kernels of a grind chain (pow_arm_kernel, pow_search_kernel, pow_finish_kernel of toyni_amd/csrc/toyni_hip.hip,
// include/toyni_hip.h 3n) themselves on the CPU through hip_sim.hpp, every GPU thread a fiber, under grid shapes and execution orders
// that a device never promises: the eight wave / lane schedules of that header, each with the workgroups in ascending and in
// DESCENDING order (descending waves and lanes with descending workgroups runs the highest thread of the grid first).
//
// TEST INFRASTRUCTURE (tests/test_sim_pow.py).  The search waits for nothing, so every order is a legal execution, and the chain must
// leave the SMALLEST accepted nonce under each of them.  The expected nonces are not computed here: the test passes the cases in and
// judges the printed results against tests/pow_model.py.
//
// Built twice: as it stands, and with -DSIM_POW_WRONG_RULE, which replaces the stop rule of pow_kernels.hpp by the classic wrong one
// ("stop as soon as anything has been found") through the macro that file offers -- the test shows that some order then returns a
// nonce that is accepted but not minimal.
//
//   sim_pow < cases        one case per line:  <hex state|-> <bits> <start> <log_tries>
//   -> RESULT <case> <grid>x<block> <schedule> <blocks-asc|blocks-desc> nonce=<v> status=<v> len=<v> state=<hex of len bytes>
//   -> launches=... hard failures=...   then DONE
#include "hip_sim.hpp"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>

#ifdef SIM_POW_WRONG_RULE
#define TOYNI_POW_STOP_RULE(candidate, best) ((void)(candidate), (best) != ~(uint64_t)0)
#endif
#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"

extern "C" {
extern uint32_t __start_hipsim_lds[] __attribute__((weak)), __stop_hipsim_lds[] __attribute__((weak));
}
void hipsim::poison_shared() {
    for (uint32_t* p = __start_hipsim_lds; p < __stop_hipsim_lds; ++p) *p = 0xDEADBEEFu;
}

// hipsim::launch with the workgroups of the grid in descending order
template <class F>
static bool launch_blocks_desc(const char* name, dim3 grid, uint32_t block, F&& body) {
    hipsim::State& s = hipsim::st();
    s.cur_name = name;
    s.cur_kernel = &s.kernels[name];
    ++s.cur_kernel->launches;
    ++s.launches;
    s.launch_failed = false;
    s.body = body;
    s.rng = 0x5EED0000ull + (uint64_t)s.sched.waves * 7919u;
    hipsim::poison_shared();
    gridDim = grid;
    blockDim = dim3(block);
    for (uint32_t bx = grid.x; bx-- > 0 && !s.launch_failed;) {
        blockIdx = dim3(bx, 0);
        hipsim::run_block(block);
    }
    return !s.launch_failed;
}

struct Shape { uint32_t grid, block; };
static const Shape SHAPES[] = {{1, 64}, {3, 64}, {4, 256}, {2, 192}};

int main() {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    hipsim::State& s = hipsim::st();
    alignas(16) static TranscriptState tr;
    alignas(8) static uint64_t nonce;
    std::string line;
    int ncase = 0;
    // one throw-away launch so that the simulator's stacks exist before launch_blocks_desc is used
    hipsim::launch("warm", "", dim3(1), 1, [] {});
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string hex;
        uint32_t bits = 0, log_tries = 0;
        unsigned long long start = 0;
        if (!(in >> hex >> bits >> start >> log_tries)) continue;
        std::vector<uint8_t> state;
        if (hex != "-")
            for (size_t i = 0; i + 1 < hex.size(); i += 2) state.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
        if (state.size() > TRANSCRIPT_CAPACITY || log_tries > POW_MAX_LOG_TRIES) return 2;
        const uint64_t tries = (uint64_t)1 << log_tries;
        for (const Shape& shape : SHAPES)
            for (int k = 0; k < hipsim::NUM_SCHEDULES; ++k)
                for (int desc = 0; desc < 2; ++desc) {
                    s.sched = hipsim::schedule_of(k);
                    memset(&tr, 0, sizeof tr);
                    memset(tr.bytes, 0x5A, sizeof tr.bytes);   // stale bytes beyond the state
                    if (!state.empty()) memcpy(tr.bytes, state.data(), state.size());
                    tr.len = (uint32_t)state.size();
                    nonce = 0x2222222222222222ull;
                    bool ok = hipsim::launch("pow_arm_kernel", "", dim3(1), TRANSCRIPT_T, [&] { pow_arm_kernel(&tr, &nonce); });
                    const auto search = [&] { pow_search_kernel(&tr, bits, (uint64_t)start, tries, &nonce); };
                    ok = ok && (desc ? launch_blocks_desc("pow_search_kernel", dim3(shape.grid), shape.block, search)
                                     : hipsim::launch("pow_search_kernel", "", dim3(shape.grid), shape.block, search));
                    ok = ok && hipsim::launch("pow_finish_kernel", "", dim3(1), TRANSCRIPT_T,
                                              [&] { pow_finish_kernel(&tr, &nonce, bits, (uint64_t)start + (tries - 1u) == ~(uint64_t)0 ? 1u : 0u); });
                    std::printf("RESULT %d %ux%u %s %s nonce=%llu status=%u len=%u state=", ncase, shape.grid, shape.block, hipsim::schedule_name(k).c_str(),
                                desc ? "blocks-desc" : "blocks-asc", (unsigned long long)nonce, tr.status, tr.len);
                    for (uint32_t i = 0; i < tr.len && i < TRANSCRIPT_CAPACITY; ++i) std::printf("%02x", tr.bytes[i]);
                    std::printf("%s\n", ok ? "" : " LAUNCH-FAILED");
                }
        ++ncase;
    }
    for (auto& kv : s.kernels) {
        s.cur_kernel = &kv.second;
        for (size_t i = 0; i < kv.second.sites.size(); ++i)
            std::printf("SITE %s:%zu %s arrivals=%llu\n", kv.first.c_str(), i, hipsim::site_text((int)i).c_str(), kv.second.sites[i].arrivals);
    }
    std::printf("launches=%llu hard failures=%llu\nDONE\n", s.launches, s.hard_failures);
    return 0;
}
