// A CPU stand-in for the few HIP names the kernel section of toyni_amd/csrc/toyni_hip.hip uses, and a scheduler that runs the
// kernels' OWN text -- the __global__ functions, barriers included -- under deliberately unfriendly wave and lane orders.
//
// TEST INFRASTRUCTURE (tests/sim/sim_kernels.cpp, tests/test_sim_schedules.py).  Host compiler in plain C++ mode; the file must be
// included BEFORE any header of toyni_amd/csrc, because it defines the host forms of TOYNI_BARRIER, TOYNI_LDS_BARRIER,
// TOYNI_WAVE_ORDER and TOYNI_UNIFORM (bb_field.hpp keeps a definition it finds).
//
// Model.  Every GPU thread is a fiber (ucontext; no OS threads, so a run is a function of its arguments alone).  Workgroups run one
// after another.  A SCHEDULE is (wave order, lane order):
//   * between two workgroup barriers the waves run one after another in the schedule's order, each all the way to the barrier (or
//     to its return) before the next one starts;
//   * inside a wave the lanes run one after another in the schedule's lane order, up to the next wave rendezvous (TOYNI_WAVE_ORDER,
//     __shfl_up) -- which the 64 lanes of that wave alone take part in -- or to the barrier;
//   * a barrier opens when every wave that has not returned has arrived.
// Ascending and descending wave orders together put every pair of waves in both orders, so a cross-wave read-after-write or
// write-after-read without a barrier between them reads stale data in one of the two.  "Stale" is what the previous workgroup left
// in the __shared__ arrays (function-local statics here), and 0xDEADBEEF at the start of every launch.
// Hard failures, whatever the outputs: lanes of one wave that disagree at a barrier (some arrived and some returned, or arrived from
// different source lines), a wave that waits where it can never be released, and a TOYNI_UNIFORM value that differs between the
// lanes of a wave (the device would silently take lane 0's).
// A synchronisation SITE is (kind, file, line) of a barrier, __syncthreads, TOYNI_WAVE_ORDER or __shfl_up; the sites of a kernel are
// numbered in order of first arrival, and one of them can be switched off (drop): the mutation that shows a site is needed.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <ucontext.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

namespace hipsim {

struct dim3 {
    uint32_t x, y, z;
    dim3(uint32_t x_ = 1, uint32_t y_ = 1, uint32_t z_ = 1) : x(x_), y(y_), z(z_) {}
};

enum SiteKind { SITE_BARRIER = 0, SITE_LDS_BARRIER = 1, SITE_SYNCTHREADS = 2, SITE_WAVE_ORDER = 3, SITE_SHFL = 4 };
inline const char* site_kind_name(int k) {
    static const char* n[] = {"barrier", "lds_barrier", "syncthreads", "wave_order", "shfl_up"};
    return n[k];
}
inline bool site_is_wave(int k) { return k == SITE_WAVE_ORDER || k == SITE_SHFL; }

struct Site {
    int kind;
    const char* file;
    int line;
    unsigned long long arrivals;
};
struct KernelSites {
    std::vector<Site> sites;
    unsigned long long launches = 0;
};

enum WaveMode { WAVES_ASC = 0, WAVES_DESC = 1, WAVES_SHUFFLE_A = 2, WAVES_SHUFFLE_B = 3 };
struct Schedule {
    int waves = WAVES_ASC;
    bool lanes_desc = false;
};
constexpr int NUM_SCHEDULES = 8;
inline Schedule schedule_of(int k) { return Schedule{k >> 1, (k & 1) != 0}; }
inline std::string schedule_name(int k) {
    static const char* w[] = {"waves-asc", "waves-desc", "waves-shuffle-a", "waves-shuffle-b"};
    return std::string(w[k >> 1]) + (k & 1 ? "/lanes-desc" : "/lanes-asc");
}

enum FiberState { F_RUNNABLE, F_WAVE, F_BARRIER, F_DONE };
struct Fiber {
    ucontext_t ctx;
    uint32_t tid = 0;
    int state = F_DONE;
    int site = -1;
    uint32_t shfl_round = 0;
    std::vector<uint64_t> uni;   // running hash after each TOYNI_UNIFORM of the current barrier interval
};

constexpr uint32_t MAX_THREADS = 1024, WAVE = 64;
constexpr size_t STACK_BYTES = 256u << 10;

struct State {
    std::map<std::string, KernelSites> kernels;
    KernelSites* cur_kernel = nullptr;
    std::string cur_name;
    Schedule sched;
    std::string drop_kernel;
    int drop_site = -1;
    unsigned long long dropped_calls = 0;
    // the run in progress
    Fiber fibers[MAX_THREADS];
    char* stacks = nullptr;
    Fiber* cur = nullptr;
    ucontext_t main_ctx;
    std::function<void()> body;
    uint32_t shfl_pub[2][MAX_THREADS];
    uint64_t rng = 0;
    // results
    unsigned long long hard_failures = 0, launches = 0, switches = 0;
    std::string last_failure;
    bool launch_failed = false;
};
inline State& st() { static State s; return s; }

}  // namespace hipsim

// the built-in variables: plain globals, rewritten at every fiber switch (one fiber runs at a time)
inline hipsim::dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace hipsim {

inline int site_index(int kind, const char* file, int line) {
    std::vector<Site>& v = st().cur_kernel->sites;
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i].line == line && v[i].kind == kind && (v[i].file == file || !strcmp(v[i].file, file))) { ++v[i].arrivals; return (int)i; }
    v.push_back(Site{kind, file, line, 1});
    return (int)v.size() - 1;
}
inline bool site_dropped(int idx) { return idx == st().drop_site && st().cur_name == st().drop_kernel; }

// a fiber gives up the processor at a synchronisation site
inline void yield_at(int kind, const char* file, int line) {
    State& s = st();
    Fiber* f = s.cur;
    if (!f) return;   // not inside a launch
    const int idx = site_index(kind, file, line);
    if (site_dropped(idx)) { ++s.dropped_calls; return; }
    f->site = idx;
    f->state = site_is_wave(kind) ? F_WAVE : F_BARRIER;
    swapcontext(&f->ctx, &s.main_ctx);
}

// __shfl_up of the scans: publish, wave rendezvous, read.  Two publication buffers: a lane that has read round k may publish round
// k + 1 before a later lane of the schedule has read round k, and cannot reach round k + 2 before every lane has arrived at k + 1.
inline int shfl_up(int v, uint32_t delta, int width, const char* file, int line) {
    State& s = st();
    Fiber* f = s.cur;
    const uint32_t buf = f->shfl_round++ & 1u, lane = f->tid & (WAVE - 1);
    (void)width;
    s.shfl_pub[buf][f->tid] = (uint32_t)v;
    yield_at(SITE_SHFL, file, line);
    return (int)s.shfl_pub[buf][lane >= delta ? f->tid - delta : f->tid];
}

// TOYNI_UNIFORM: the value goes through unchanged; (site, value) is folded into the lane's running hash
inline uint32_t uniform_value(const char* file, int line, uint32_t v) {
    Fiber* f = st().cur;
    if (!f) return v;
    uint64_t h = f->uni.empty() ? 0x9E3779B97F4A7C15ull : f->uni.back();
    h ^= ((uint64_t)(uint32_t)line << 32) | v;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
    for (const char* c = file + (strlen(file) > 8 ? strlen(file) - 8 : 0); *c; ++c) h = (h ^ (uint8_t)*c) * 0x100000001B3ull;
    f->uni.push_back(h);
    return v;
}

inline void fail(const std::string& what) {
    State& s = st();
    ++s.hard_failures;
    s.launch_failed = true;
    s.last_failure = s.cur_name + ": " + what;
    printf("HARD FAILURE %s [block %u,%u]\n", s.last_failure.c_str(), blockIdx.x, blockIdx.y);
}

inline void fiber_main() {
    State& s = st();
    s.body();
    s.cur->state = F_DONE;
    swapcontext(&s.cur->ctx, &s.main_ctx);   // never resumed
}

inline void switch_to(Fiber& f) {
    State& s = st();
    s.cur = &f;
    threadIdx.x = f.tid;
    ++s.switches;
    swapcontext(&s.main_ctx, &f.ctx);
    s.cur = nullptr;
}

inline uint64_t next_random() {
    uint64_t z = (st().rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

inline std::string site_text(int idx) {
    const Site& x = st().cur_kernel->sites[idx];
    const char* base = strrchr(x.file, '/');
    return std::string(site_kind_name(x.kind)) + "@" + (base ? base + 1 : x.file) + ":" + std::to_string(x.line);
}

// the lanes of a wave took the same TOYNI_UNIFORM values in the same order (a lane that returned early: a prefix of them)
inline bool uniform_agree(uint32_t first, uint32_t count) {
    State& s = st();
    const Fiber* ref = &s.fibers[first];
    for (uint32_t l = 0; l < count; ++l)
        if (s.fibers[first + l].uni.size() > ref->uni.size()) ref = &s.fibers[first + l];
    bool ok = true;
    for (uint32_t l = 0; l < count; ++l) {
        const Fiber& f = s.fibers[first + l];
        if (!f.uni.empty() && f.uni.back() != ref->uni[f.uni.size() - 1]) ok = false;
    }
    for (uint32_t l = 0; l < count; ++l) s.fibers[first + l].uni.clear();
    return ok;
}

// Runs wave w up to a workgroup barrier or to its return.  false: hard failure.
inline bool run_wave(uint32_t w, uint32_t nthreads) {
    State& s = st();
    const uint32_t first = w * WAVE, count = nthreads - first < WAVE ? nthreads - first : WAVE;
    while (true) {
        for (uint32_t k = 0; k < count; ++k) {
            Fiber& f = s.fibers[first + (s.sched.lanes_desc ? count - 1 - k : k)];
            if (f.state == F_RUNNABLE) switch_to(f);
        }
        uint32_t nwave = 0, nbar = 0, ndone = 0;
        int site = -1;
        bool same_site = true;
        for (uint32_t l = 0; l < count; ++l) {
            const Fiber& f = s.fibers[first + l];
            if (f.state == F_DONE) { ++ndone; continue; }
            if (f.state == F_WAVE) ++nwave; else ++nbar;
            if (site < 0) site = f.site;
            else if (site != f.site) same_site = false;
        }
        if (nwave && nbar) { fail("wave " + std::to_string(w) + " waits where it can never be released: some lanes at a wave rendezvous, some at a barrier"); return false; }
        if (!same_site) { fail("lanes of wave " + std::to_string(w) + " arrived from different source lines (" + site_text(site) + " and another)"); return false; }
        if (nwave) {   // (lanes that have returned take no part in a wave rendezvous)
            for (uint32_t l = 0; l < count; ++l)
                if (s.fibers[first + l].state == F_WAVE) s.fibers[first + l].state = F_RUNNABLE;
            continue;
        }
        if (nbar && ndone) { fail("lanes of wave " + std::to_string(w) + " disagree at " + site_text(site) + ": some arrived, some returned"); return false; }
        if (!uniform_agree(first, count)) { fail("a TOYNI_UNIFORM value differs between the lanes of wave " + std::to_string(w)); return false; }
        return true;
    }
}

inline void run_block(uint32_t nthreads) {
    State& s = st();
    const uint32_t nw = (nthreads + WAVE - 1) / WAVE;
    for (uint32_t t = 0; t < nthreads; ++t) {
        Fiber& f = s.fibers[t];
        f.tid = t;
        f.state = F_RUNNABLE;
        f.site = -1;
        f.shfl_round = 0;
        f.uni.clear();
        getcontext(&f.ctx);
        f.ctx.uc_stack.ss_sp = s.stacks + (size_t)t * STACK_BYTES;
        f.ctx.uc_stack.ss_size = STACK_BYTES;
        f.ctx.uc_link = nullptr;
        makecontext(&f.ctx, fiber_main, 0);
    }
    std::vector<uint32_t> order(nw);
    while (true) {
        for (uint32_t w = 0; w < nw; ++w) order[w] = s.sched.waves == WAVES_DESC ? nw - 1 - w : w;
        if (s.sched.waves >= WAVES_SHUFFLE_A)   // re-drawn at every barrier interval
            for (uint32_t w = nw; w > 1; --w) { const uint32_t j = (uint32_t)(next_random() % w); const uint32_t t = order[w - 1]; order[w - 1] = order[j]; order[j] = t; }
        bool any_waiting = false;
        for (uint32_t k = 0; k < nw; ++k) {
            const uint32_t w = order[k];
            if (s.fibers[w * WAVE].state == F_DONE) continue;   // the wave returned (all its lanes: run_wave saw to that)
            if (!run_wave(w, nthreads)) return;
            if (s.fibers[w * WAVE].state != F_DONE) any_waiting = true;
        }
        if (!any_waiting) return;
        // every wave that has not returned has arrived: the barrier opens
        for (uint32_t t = 0; t < nthreads; ++t)
            if (s.fibers[t].state == F_BARRIER) s.fibers[t].state = F_RUNNABLE;
    }
}

void poison_shared();   // sim_kernels.cpp: 0xDEADBEEF into every __shared__ array

// name: the kernel's name (sites are numbered per name); inst: the instantiation, for the printed list
template <class F>
inline bool launch(const char* name, const std::string& inst, dim3 grid, uint32_t block, F&& body) {
    State& s = st();
    if (!s.stacks) {
        s.stacks = (char*)mmap(nullptr, STACK_BYTES * MAX_THREADS, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (s.stacks == (char*)MAP_FAILED || block > MAX_THREADS) { perror("stacks"); exit(2); }
    }
    (void)inst;
    s.cur_name = name;
    s.cur_kernel = &s.kernels[name];
    ++s.cur_kernel->launches;
    ++s.launches;
    s.launch_failed = false;
    s.body = body;
    s.rng = 0x5EED0000ull + (uint64_t)s.sched.waves * 7919u;
    poison_shared();
    gridDim = grid;
    blockDim = dim3(block);
    for (uint32_t by = 0; by < grid.y && !s.launch_failed; ++by)
        for (uint32_t bx = 0; bx < grid.x && !s.launch_failed; ++bx) {
            blockIdx = dim3(bx, by);
            run_block(block);
        }
    return !s.launch_failed;
}

}  // namespace hipsim

// ---- the HIP names of the kernel section ----
using hipsim::dim3;
struct alignas(16) uint4 { uint32_t x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
inline uint32_t atomicOr(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o | v; return o; }

#define __global__ static
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __align__(n) __attribute__((aligned(n)))
#define __shared__ static __attribute__((section("hipsim_lds")))
#define __HIP_MEMORY_SCOPE_SYSTEM 0
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n((p), (v), (order))
#define __syncthreads() hipsim::yield_at(hipsim::SITE_SYNCTHREADS, __FILE__, __LINE__)
#define __shfl_up(v, delta, width) hipsim::shfl_up((v), (delta), (width), __FILE__, __LINE__)
#define TOYNI_BARRIER() hipsim::yield_at(hipsim::SITE_BARRIER, __FILE__, __LINE__)
#define TOYNI_LDS_BARRIER() hipsim::yield_at(hipsim::SITE_LDS_BARRIER, __FILE__, __LINE__)
#define TOYNI_WAVE_ORDER() hipsim::yield_at(hipsim::SITE_WAVE_ORDER, __FILE__, __LINE__)
#define TOYNI_UNIFORM(x) hipsim::uniform_value(__FILE__, __LINE__, (uint32_t)(x))
