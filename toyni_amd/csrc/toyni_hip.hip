// libtoyni_hip.so -- gfx950 kernels + C ABI (include/toyni_hip.h).
// Replaces cuda/ntt_kernel.cu of the reference; written for CDNA4 only (wave64, 160 KiB LDS, no MFMA:
// the path is integer modular arithmetic).  Kernel bodies live in ntt_kernels.hpp.
// TOYNI_KERNEL_TEXT_ONLY (tests/sim; never a product build): the kernel section alone -- no HIP runtime, no launch registry, no
// context and no C ABI -- for a translation unit that supplies the handful of HIP names the kernels use and runs them on the CPU.
#ifndef TOYNI_KERNEL_TEXT_ONLY
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#ifdef TOYNI_TOOLS
#include "toyni_hip_tools.h"
#endif
#endif  // TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.h"  // include/toyni_hip.h: -I include here; next to this file in a crate's hip/ directory
#include "ntt_plan.hpp"
#include "merkle_kernels.hpp"
#include "prover_kernels.hpp"
#include "transcript_kernels.hpp"
#include "pow_kernels.hpp"
#include "dz_kernels.hpp"
#include "dc_kernels.hpp"
#include "fib_dz_kernels.hpp"

using namespace toyni;

#ifndef TOYNI_KERNEL_TEXT_ONLY
// ------------------------------------------------------------------------------------------------
// launch registry (toyni_launched_kernels, include/toyni_hip.h section 4)
// ------------------------------------------------------------------------------------------------
// Every launch site of this translation unit goes through the macro below: the FIRST launch of a site resolves the kernel's symbol
// (hipKernelNameRefByPtr) and files it in an in-memory list; every later one costs a relaxed load of a site-local flag.
// tests/test_zz_kernel_coverage.py compares the list of a finished GPU test session with the kernel symbols of the shipped binary, so
// "every kernel the launcher can pick has been through the parity tests" is a test, not a sentence.  The library itself
// writes NO file (rounds 3-4 appended to $TOYNI_LAUNCH_LOG from here: an environment-driven fopen in the product): child
// processes of a test session dump toyni_launched_kernels() at exit through the test harness (tests/_hooks/sitecustomize.py for Python
// children, tests/cpp/launch_dump.hpp for the compiled hosts).
namespace launch_registry {
inline std::mutex& mu() { static std::mutex m; return m; }
inline std::vector<std::string>& names() { static std::vector<std::string> v; return v; }
inline bool note(const void* host_fn) {
    const char* nm = hipKernelNameRefByPtr(host_fn, nullptr);
    if (!nm) { (void)hipGetLastError(); return false; }   // not filed: the site tries again at its next launch
    std::lock_guard<std::mutex> lk(mu());
    for (const auto& s : names())
        if (s == nm) return true;
    names().push_back(nm);
    return true;
}
}  // namespace launch_registry
#undef hipLaunchKernelGGL
// (the site flag is set only AFTER the symbol is in the list -- a concurrent toyni_launched_kernels() never sees a site marked whose
// name is missing; two threads racing through a site's first launch both call note(), which files a name once)
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...)                                      \
    do {                                                                                                 \
        static std::atomic<bool> _toyni_site_seen{false};                                                \
        if (!_toyni_site_seen.load(std::memory_order_acquire)) {                                         \
            if (launch_registry::note(reinterpret_cast<const void*>(kernel)))                            \
                _toyni_site_seen.store(true, std::memory_order_release);                                 \
        }                                                                                                \
        kernel<<<(grid), (block), (shmem), (stream)>>>(__VA_ARGS__);                                     \
    } while (0)

#define HIPCHK(expr)                                 \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return (int)_e;          \
    } while (0)
#endif  // TOYNI_KERNEL_TEXT_ONLY

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// Persistent workgroups: workgroup b runs tiles tile_order(b), tile_order(b + grid), ...  Two-step passes are
// software-pipelined around one rule: vmcnt retires loads AND stores in issue order, so a load that is waited for
// after a tile's 32 HBM stores were issued would wait for those stores to be acknowledged.  Hence, in the steady state,
//   * the step-1 stage twiddles live in LDS (copied once per workgroup; LDS reads count on lgkmcnt),
//   * as soon as a tile's registers are parked in LDS they are refilled with the NEXT tile's HBM loads (first PF of
//     them; the rest at the top of the next iteration), and the next tile's twiddle-seed lookups are issued right
//     behind them -- all of it BEFORE the current tile's stores, in flight across the barrier and the whole of step 2.
// The barriers are raw s_barrier with an explicit LDS-only wait: __syncthreads() would also drain vmcnt.
template <class P> struct PassKindOf;
template <int K, int A, int B, int C, bool N, int Q, bool S> struct PassKindOf<Pass<K, A, B, C, N, Q, S>> { static constexpr int value = K; };
template <class P> constexpr int kind_of() { return PassKindOf<P>::value; }

// LZ > 0: first pass of a low-degree extension -- the input holds only the leading n >> LZ words of every transform
// (the zero padding is implied): fewer loads, and the top LZ stages of step 1 degenerate to one multiply per output.
template <class P, int PF, int LZ = 0>
__global__ void __launch_bounds__(P::T, P::MIN_WAVES) ntt_pass_kernel(const PassArgs a, const uint32_t ntiles) {
    __shared__ uint32_t lds[(P::LDS_WORDS + P::TW1_WORDS + P::TW3_WORDS) ? (P::LDS_WORDS + P::TW1_WORDS + P::TW3_WORDS) : 1];
    const uint32_t tid = threadIdx.x;
    if constexpr (!P::TWO_STEP) {
        static_assert(LZ == 0, "single-step passes take whole inputs");
        for (uint32_t v = blockIdx.x; v < ntiles; v += gridDim.x) P::phase1(a, P::tile_order(v, ntiles), tid, lds);
    } else {
        constexpr uint32_t NPF = PF < 0 ? 0u : ((uint32_t)PF > P::E1 ? P::E1 : (uint32_t)PF);
        uint32_t v = blockIdx.x;
        if (v >= ntiles) return;
        uint32_t* lds_tw1 = lds + P::LDS_WORDS;
        uint32_t* lds_tw3 = lds_tw1 + P::TW1_WORDS;   // radix-4 companion of the step-1 stage twiddles
        uint32_t x[P::E1];
        typename P::Tile t = P::tile_of(a, P::tile_order(v, ntiles));
        P::template load_tile<0, NPF, LZ>(a, t, tid, x);
        typename P::SeedsRaw raw = P::seeds_issue(a, t, tid);
        typename P::InSeedRaw inraw = P::in_seed_issue(a, t, tid);
        const typename P::Uniform uni = P::load_uniform(a);  // step-2 twiddles, SGPR-resident for the whole loop
        for (uint32_t j = tid; j < P::TW1_WORDS; j += P::T) lds_tw1[j] = P::tw1_global(a)[j];
        for (uint32_t j = tid; j < P::TW3_WORDS; j += P::T) lds_tw3[j] = P::tw3_global(a)[j];
        TOYNI_WAIT_VMEM0();  // the first tile's loads have landed: the loop is entered with no load pending on any path
        __syncthreads();
        // Launch-invariant seeds (column passes, PassArgs::seeds_invariant): the seeds depend on the tile through its column index
        // alone, and where the launcher has established that this workgroup never leaves its column tile they are finished here,
        // once, and stay in registers across the loop -- no table gather and no seed product per tile.  Otherwise (uniform branch;
        // a constant for the row kinds) every tile looks its own up, a tile ahead, as before.
        const bool hoist = kind_of<P>() == KIND_COL && !P::SLAB && a.seeds_invariant != 0u;
        typename P::Seeds seeds = P::seeds_finish(a, raw);
        uint32_t inseed = P::in_seed_finish(a, inraw);
        while (true) {
            // The tile's loads (prefetch + seed lookups) were issued BEFORE the previous tile's E1 stores, and vmcnt
            // retires in issue order: allowing exactly the E1 youngest operations to stay outstanding retires every
            // load while the stores keep draining in the background.  (Ragged single-pass row tiles issue fewer
            // stores, so they wait for everything.)  With the seed lookups hoisted the count stands: the youngest E1
            // operations are still exactly the previous tile's stores, there are just fewer loads in front of them.
            static_assert(P::G2 * P::E2 == P::E1 && P::E1 <= 63, "stores per tile per thread");
            if constexpr (kind_of<P>() != KIND_ROW_N) TOYNI_WAIT_VMEM_ALLOW(P::E1);
            else TOYNI_WAIT_VMEM0();
            P::template load_tile<NPF, P::E1, LZ>(a, t, tid, x);
            if (!hoist) inseed = P::in_seed_finish(a, inraw);
            P::template in_scale_by<LZ>(a, inseed, x);  // forward coset FFT only (uniform branch)
            P::template step1<LZ>(a, t, tid, x, lds, uni, lds_tw1, lds_tw3);
            if (!hoist) seeds = P::seeds_finish(a, raw);
#pragma unroll
            for (uint32_t g = 0; g < P::G2; ++g) { TOYNI_PIN(seeds.g[g].a0); TOYNI_PIN(seeds.g[g].g); }  // materialised HERE
            TOYNI_SCHED_FENCE();
            const uint32_t vn = v + gridDim.x;
            const bool more = vn < ntiles;  // uniform
            typename P::Tile tn = t;
            if (more) {
                tn = P::tile_of(a, P::tile_order(vn, ntiles));
                P::template load_tile<0, NPF, LZ>(a, tn, tid, x);  // prefetch
                if (!hoist) {
                    raw = P::seeds_issue(a, tn, tid);          // and the next tile's seed lookups, still ahead of the stores
                    inraw = P::in_seed_issue(a, tn, tid);
                }
            }
            TOYNI_SCHED_FENCE();
            TOYNI_LDS_BARRIER();  // this wave's LDS writes have landed; then the rendezvous
            TOYNI_SCHED_FENCE();
            P::step2(a, t, tid, lds, seeds, uni);
            if (!more) break;
            TOYNI_SCHED_FENCE();
            TOYNI_BARRIER();  // every wave has its step-2 LDS reads in registers before the tile is overwritten
            TOYNI_SCHED_FENCE();
            t = tn;
            v = vn;
        }
    }
}

// Three-step passes (Pass3, ntt_kernels.hpp): the latency configuration.  Persistent over its tiles without a software
// prefetch: with 16 elements per thread the kernel is light on registers, and the launches it serves have at most a few
// tiles per CU.  The step-3 twiddle lookups are issued with the tile's loads and stay in flight across both barriers.
template <class P, int LZ = 0>
__global__ void __launch_bounds__(P::T, P::MIN_WAVES) ntt_pass3_kernel(const PassArgs a, const uint32_t ntiles) {
    __shared__ uint32_t lds[P::LDS_WORDS + P::TW_WORDS];
    const uint32_t tid = threadIdx.x;
    uint32_t v = blockIdx.x;
    if (v >= ntiles) return;
    uint32_t* lds_tw = lds + P::LDS_WORDS;
    // the stage table's way into LDS overlaps the first tile's loads: both are issued before either is waited for (a lone
    // transform is one tile per workgroup, and two memory latencies in a row were a third of such a launch)
    constexpr uint32_t TW_REGS = (P::TW_WORDS + P::T - 1) / P::T;
    uint32_t tw_regs[TW_REGS];
#pragma unroll
    for (uint32_t k = 0; k < TW_REGS; ++k) {
        const uint32_t j = tid + k * P::T;
        tw_regs[k] = j < P::TW_WORDS ? P::tw_global(a)[j] : 0u;
    }
    const typename P::Uniform uni = P::load_uniform(a);
    bool first = true;
    while (true) {
        const typename P::Tile t = P::tile_of(a, P::tile_order(v, ntiles));
        uint32_t x[P::E];
        P::template load_tile<LZ>(a, t, tid, x);
        const typename P::InSeedRaw inraw = P::in_seed_issue(a, t, tid);
        const typename P::SeedsRaw raw = P::seeds_issue(a, t, tid);
        if (first) {
#pragma unroll
            for (uint32_t k = 0; k < TW_REGS; ++k) {
                const uint32_t j = tid + k * P::T;
                if (j < P::TW_WORDS) lds_tw[j] = tw_regs[k];
            }
            TOYNI_SCHED_FENCE();
            TOYNI_LDS_BARRIER();
            TOYNI_SCHED_FENCE();
            first = false;
        }
        P::template step1<LZ>(a, inraw, tid, x, lds, lds_tw + ((1u << P::LLO) - P::E3));
        TOYNI_SCHED_FENCE();
        TOYNI_LDS_BARRIER();
        TOYNI_SCHED_FENCE();
        P::step2(tid, lds, lds_tw);
        TOYNI_SCHED_FENCE();
        TOYNI_LDS_BARRIER();
        TOYNI_SCHED_FENCE();
        P::step3(a, t, tid, lds, P::seeds_finish(a, raw), uni);
        v += gridDim.x;
        if (v >= ntiles) break;
        TOYNI_SCHED_FENCE();
        TOYNI_BARRIER();  // every wave has its step-3 LDS reads in registers before the tile is overwritten
        TOYNI_SCHED_FENCE();
    }
}

// Streaming three-step passes (Pass3 with 32 elements per thread, round 5): the pipeline of ntt_pass_kernel around three steps.
// The next tile's loads (and its seed lookups) are issued as soon as step 1 has parked the registers in LDS -- ahead of this
// tile's E stores, so that the counted vmcnt wait at the top of the loop retires them while the stores drain -- and stay in flight
// across both data barriers and steps 2 and 3.  The step-1 twiddle slices live in LDS, the step-2 twiddles in registers.
template <class P, int LZ = 0>
__global__ void __launch_bounds__(P::T, P::MIN_WAVES) ntt_pass3s_kernel(const PassArgs a, const uint32_t ntiles) {
    static_assert(P::STREAM && P::G3 * P::E3 == P::E && P::E <= 63, "stores per tile per thread");
    __shared__ uint32_t lds[P::LDS_WORDS + P::TW1S_WORDS + P::TW3S_WORDS];
    const uint32_t tid = threadIdx.x;
    uint32_t v = blockIdx.x;
    if (v >= ntiles) return;
    uint32_t* lds_tw1 = lds + P::LDS_WORDS;
    uint32_t* lds_tw3 = lds_tw1 + P::TW1S_WORDS;
    uint32_t x[P::E];
    typename P::Tile t = P::tile_of(a, P::tile_order(v, ntiles));
    P::template load_tile<LZ>(a, t, tid, x);
    typename P::SeedsRaw raw = P::seeds_issue(a, t, tid);
    typename P::InSeedRaw inraw = P::in_seed_issue(a, t, tid);
    const typename P::Uniform uni = P::load_uniform(a);
    const typename P::Tw2 tw2 = P::load_tw2(a, tid);
    for (uint32_t j = tid; j < P::TW1S_WORDS; j += P::T) lds_tw1[j] = P::tw1s_global(a)[j];
    for (uint32_t j = tid; j < P::TW3S_WORDS; j += P::T) lds_tw3[j] = P::tw3s_global(a)[j];
    TOYNI_WAIT_VMEM0();
    __syncthreads();
    while (true) {
        TOYNI_WAIT_VMEM_ALLOW(P::E);   // this tile's loads were issued before the previous tile's E stores
        P::template step1<LZ>(a, inraw, tid, x, lds, lds_tw1, lds_tw3);
        typename P::Seeds seeds = P::seeds_finish(a, raw);
        TOYNI_SCHED_FENCE();
        const uint32_t vn = v + gridDim.x;
        const bool more = vn < ntiles;  // uniform
        typename P::Tile tn = t;
        if (more) {
            tn = P::tile_of(a, P::tile_order(vn, ntiles));
            P::template load_tile<LZ>(a, tn, tid, x);   // prefetch
            raw = P::seeds_issue(a, tn, tid);
            inraw = P::in_seed_issue(a, tn, tid);
        }
        TOYNI_SCHED_FENCE();
        if constexpr (P::WAVE_LOCAL2) TOYNI_WAVE_ORDER();   // step 2 reads what this wave itself wrote: program order suffices
        else TOYNI_LDS_BARRIER();
        TOYNI_SCHED_FENCE();
        P::step2_regs(tid, lds, tw2);
        TOYNI_SCHED_FENCE();
        TOYNI_LDS_BARRIER();
        TOYNI_SCHED_FENCE();
        P::step3(a, t, tid, lds, seeds, uni);
        if (!more) break;
        TOYNI_SCHED_FENCE();
        TOYNI_BARRIER();  // every wave has its step-3 LDS reads in registers before the tile is overwritten
        TOYNI_SCHED_FENCE();
        t = tn;
        v = vn;
    }
}

// Single-sweep transform for n = 2^11 .. 2^15 (LdsPass, ntt_kernels.hpp): one 1024-thread workgroup per CU keeps a tile of
// 32 rows x 1024 words in LDS through all three phases; persistent over the tiles of the batch.  The next tile's loads
// are issued as soon as phase A has parked the registers in LDS, ahead of this tile's stores (vmcnt retires in issue
// order, see above); a tile that has a successor is never ragged, so exactly E stores follow every prefetch.
template <class L>
__global__ void __launch_bounds__(L::T, 4) ntt_lds_kernel(const LdsArgs g, const uint32_t ntiles) {
    __shared__ uint32_t lds[L::LDS_WORDS + L::TW1_WORDS];
    const uint32_t tid = threadIdx.x;
    uint32_t tile = blockIdx.x;
    if (tile >= ntiles) return;
    uint32_t* lds_tw1 = lds + L::LDS_WORDS;
    uint32_t x[L::E];
    L::loadA(g, tile, tid, x);
    const typename L::Seeds seeds = L::seedsA(g, tid);
    const typename L::Uniform uni = L::load_uniform(g);
    for (uint32_t j = tid; j < L::TW1_WORDS; j += L::T) lds_tw1[j] = L::tw1_global(g)[j];
    TOYNI_WAIT_VMEM0();
    __syncthreads();
    while (true) {
        TOYNI_WAIT_VMEM_ALLOW(L::E);  // the tile's loads were issued before the previous tile's E stores
        L::phaseA(g, tid, x, seeds, uni, lds);
        TOYNI_SCHED_FENCE();
        const uint32_t next = tile + gridDim.x;
        const bool more = next < ntiles;  // uniform
        if (more) L::loadA(g, next, tid, x);  // prefetch
        TOYNI_SCHED_FENCE();
        TOYNI_LDS_BARRIER();
        TOYNI_SCHED_FENCE();
        L::phaseB(tid, lds, lds_tw1);
        TOYNI_SCHED_FENCE();
        TOYNI_LDS_BARRIER();
        TOYNI_SCHED_FENCE();
        L::phaseC(g, tile, tid, lds, uni);
        if (!more) break;
        TOYNI_SCHED_FENCE();
        TOYNI_BARRIER();  // phase C's LDS reads are in registers before the tile is overwritten
        TOYNI_SCHED_FENCE();
        tile = next;
    }
}

// n = 2^11 in one sweep, one wave per transform (Row2048, ntt_kernels.hpp): no workgroup barrier after the twiddle slices are in LDS.
// A wave walks rows w, w + (waves in the grid), ...; the next row's 32 loads are issued as soon as step 1 has parked the registers
// in the wave's LDS slice, ahead of this row's 32 stores, so the counted vmcnt wait at the top retires them while the stores drain.
template <bool NT>
__global__ void __launch_bounds__(Row2048::T, 4) ntt_row2048_kernel(const PassArgs a) {
    using R = Row2048;
    __shared__ uint32_t lds[R::LDS_WORDS + R::TW1_WORDS + R::TW3_WORDS + R::TW2_WORDS];
    const uint32_t tid = threadIdx.x, l = tid & 63u;
    const uint32_t wave = TOYNI_UNIFORM(tid >> 6);
    uint32_t* lds_tw1 = lds + R::LDS_WORDS;
    uint32_t* lds_tw3 = lds_tw1 + R::TW1_WORDS;
    uint32_t* lds_tw2 = lds_tw3 + R::TW3_WORDS;
    uint32_t* row_lds = lds + wave * R::ROW_WORDS;
    for (uint32_t j = tid; j < R::TW1_WORDS; j += R::T) lds_tw1[j] = R::tw1_global(a)[j];
    for (uint32_t j = tid; j < R::TW3_WORDS; j += R::T) lds_tw3[j] = R::tw3_global(a)[j];
    if (tid < R::TW2_WORDS) lds_tw2[tid] = R::tw2_global(a)[tid];
    const uint64_t stride = (uint64_t)gridDim.x * R::WAVES;
    uint64_t row = (uint64_t)blockIdx.x * R::WAVES + wave;
    uint32_t x[R::E];
    const bool any = row < a.rows_total;   // wave-uniform
    if (any) R::template load_row<NT>(a, row, l, x);
    const R::Consts c = R::consts(a);
    TOYNI_WAIT_VMEM0();
    __syncthreads();                       // the twiddle slices: the only data the waves of a workgroup share
    if (!any) return;
    while (true) {
        TOYNI_WAIT_VMEM_ALLOW(R::E);       // this row's loads were issued before the previous row's E stores
        R::step1(a, l, x, row_lds, lds_tw1, lds_tw3);
        TOYNI_SCHED_FENCE();
        const uint64_t next = row + stride;
        const bool more = next < a.rows_total;  // wave-uniform
        if (more) R::template load_row<NT>(a, next, l, x);   // prefetch
        TOYNI_SCHED_FENCE();
        TOYNI_WAVE_ORDER();                // steps 2 and 3 read what this wave itself wrote: program order suffices (LDS operations of a wave execute in order)
        R::step2(l, row_lds, lds_tw2);
        TOYNI_WAVE_ORDER();
        R::template step3<NT>(a, c, row, l, row_lds);
        if (!more) break;
        TOYNI_WAVE_ORDER();
        row = next;
    }
}

// n = 2^12 in one sweep, two waves per transform (Row4096): the workgroup walks tiles of eight rows in lockstep (the two waves of a row
// meet at workgroup barriers); the next tile's loads are issued behind step 1, ahead of this tile's stores.  Rows beyond the batch
// (a ragged last tile) skip their loads, arithmetic and stores but take part in every barrier.
template <bool NT>
__global__ void __launch_bounds__(Row4096::T, 4) ntt_row4096_kernel(const PassArgs a, const uint32_t ntiles) {
    using R = Row4096;
    __shared__ uint32_t lds[R::LDS_WORDS + R::TW1_WORDS + R::TW2_WORDS];
    const uint32_t tid = threadIdx.x, tau = tid & 127u;
    const uint32_t rho = TOYNI_UNIFORM(tid >> 7);
    uint32_t* lds_tw1 = lds + R::LDS_WORDS;
    uint32_t* lds_tw2 = lds_tw1 + R::TW1_WORDS;
    uint32_t* row_lds = lds + rho * R::ROW_WORDS;
    uint32_t v = blockIdx.x;
    if (v >= ntiles) return;
    for (uint32_t j = tid; j < R::TW1_WORDS; j += R::T) lds_tw1[j] = R::tw1_global(a)[j];
    if (tid < R::TW2_WORDS) lds_tw2[tid] = R::tw2_global(a)[tid];
    uint32_t x[R::E];
    uint64_t row = (uint64_t)v * R::ROWS + rho;
    bool valid = row < a.rows_total;       // wave-uniform
    if (valid) R::template load_row<NT>(a, row, tau, x);
    const R::Consts c = R::consts(a);
    TOYNI_WAIT_VMEM0();
    __syncthreads();
    while (true) {
        TOYNI_WAIT_VMEM_ALLOW(R::E);       // this tile's loads were issued before the previous tile's E stores
        if (valid) R::step1(a, tau, x, row_lds, lds_tw1);
        TOYNI_SCHED_FENCE();
        const uint32_t vn = v + gridDim.x;
        const bool more = vn < ntiles;     // uniform
        const uint64_t row_n = (uint64_t)vn * R::ROWS + rho;
        const bool valid_n = more && row_n < a.rows_total;
        if (valid_n) R::template load_row<NT>(a, row_n, tau, x);   // prefetch
        TOYNI_SCHED_FENCE();
        TOYNI_LDS_BARRIER();
        TOYNI_SCHED_FENCE();
        if (valid) R::step2(tau, row_lds, lds_tw2);
        TOYNI_SCHED_FENCE();
        TOYNI_LDS_BARRIER();
        TOYNI_SCHED_FENCE();
        if (valid) R::template step3<NT>(a, c, row, tau, row_lds);
        if (!more) break;
        TOYNI_SCHED_FENCE();
        TOYNI_BARRIER();                   // the pair's step-3 LDS reads are in registers before the row is overwritten
        TOYNI_SCHED_FENCE();
        v = vn;
        row = row_n;
        valid = valid_n;
    }
}

__global__ void __launch_bounds__(256) narrow_kernel(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) out[i] = narrow_u64(in[i]);
}

// narrow + "Cannot invert zero" check of the fold's points (src/babybear.rs:112): *flag becomes 1 if any reduced point is 0
__global__ void __launch_bounds__(256) narrow_nonzero_kernel(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, size_t count,
                                                              uint32_t* __restrict__ flag) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    bool any_zero = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const uint32_t v = narrow_u64(in[i]);
        out[i] = v;
        any_zero |= v == 0u;
    }
    if (any_zero) atomicOr(flag, 1u);
}

__global__ void __launch_bounds__(256) widen_kernel(const uint32_t* __restrict__ in, uint64_t* __restrict__ out, size_t count) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) out[i] = in[i];
}

// 4-step twiddle: data[r][k] *= w_n^(+-(row0 + r) k), r < rows, k < row_len (two-level domain table of the ctx)
__global__ void __launch_bounds__(256) fourstep_twiddle_kernel(uint32_t* __restrict__ data, uint64_t total, uint32_t log_len, uint32_t row0,
                                                                const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi, uint32_t lowbits) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lmask = (1u << lowbits) - 1u, kmask = (1u << log_len) - 1u;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t k = (uint32_t)g & kmask;
        const uint32_t e = (row0 + (uint32_t)(g >> log_len)) * k;  // < n <= 2^27
        const uint32_t w = mont_mul(hi[e >> lowbits], lo[e & lmask]);
        data[g] = mont_mul(data[g], w);
    }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // what the non-temporal builtins accept for 16-byte accesses

// slab relayout (ntt_kernels.hpp): four consecutive output words per thread, 16-byte accesses on both sides (W >= 32).
// Round 5: four quads in flight per thread and non-temporal accesses (the data is read once and written once, 512 MiB each way at
// n = 2^27).  With one 16-byte load outstanding per thread a CU had 32 KiB in flight and the sweep moved 2.45 TB/s
// (profiles/r04_bench_slab_2p27.json); the inverse form's twiddle is one table lookup pair per quad and a running product with
// w_n^-k1 (the exponent k1 j' is linear in the column) instead of four independent lookups.
__device__ __forceinline__ uint4 relayout_quad(const RelayoutArgs& a, uint4 v, uint32_t e0, uint32_t de) {
    if (!a.inverse) return v;
    const uint32_t lmask = (1u << a.lowbits) - 1u;
    uint32_t tw = mont_mul(a.hi[e0 >> a.lowbits], a.lo[e0 & lmask]);
    const uint32_t g = mont_mul(a.hi[de >> a.lowbits], a.lo[de & lmask]);   // w_n^-k1: the factor between neighbouring columns
    uint4 r;
    r.x = mont_mul(v.x, tw); tw = mont_mul_lazy(tw, g);
    r.y = mont_mul(v.y, tw); tw = mont_mul_lazy(tw, g);
    r.z = mont_mul(v.z, tw); tw = mont_mul_lazy(tw, g);
    r.w = mont_mul(v.w, tw);
    return r;
}
__global__ void __launch_bounds__(256) slab_relayout_kernel(const RelayoutArgs a, uint64_t quads) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; q + 3 * stride < quads; q += 4 * stride) {
        u32x4 v[4];
        uint32_t e0[4], e1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t src = relayout_src(a, 4 * (q + u * stride), e0[u]);
            (void)relayout_src(a, 4 * (q + u * stride) + 1, e1[u]);
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.in + src));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint4 r = relayout_quad(a, make_uint4(v[u].x, v[u].y, v[u].z, v[u].w), e0[u], e1[u] - e0[u]);
            u32x4 o;
            o.x = r.x; o.y = r.y; o.z = r.z; o.w = r.w;
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(a.out + 4 * (q + u * stride)));
        }
    }
    for (; q < quads; q += stride) {
        uint32_t e0, e1;
        const uint64_t src = relayout_src(a, 4 * q, e0);
        (void)relayout_src(a, 4 * q + 1, e1);
        const uint4 v = *reinterpret_cast<const uint4*>(a.in + src);
        *reinterpret_cast<uint4*>(a.out + 4 * q) = relayout_quad(a, v, e0, e1 - e0);
    }
}

// roots_of_unity_domain / BabyBearDomain::elements (src/ntt.rs:69-81, src/math/domain.rs:61-69): out[i] = shift * w_m^i, the
// reference's serial multiply chain as independent two-level table lookups (w_m^i = w_n^(i << log_step), forward domain table)
__global__ void __launch_bounds__(256) domain_elements_kernel(uint32_t* __restrict__ out, uint64_t m, uint32_t shift, const SubDomain dom) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        // subdomain_mont = Montgomery form of w_m^i; times the PLAIN shift leaves the plain product shift * w_m^i
        out[i] = mont_mul(subdomain_mont(dom, (uint32_t)i), shift);
    }
}


// whole quads behind 16-byte aligned pointers: the condition under which the structured folds take 16-byte accesses (the entry points
// accept any 4-byte aligned pointer; a layer of the fold-layers loop starts wherever the one before it ended)
__host__ __device__ __forceinline__ bool fold_quads(const uint32_t* evals, const uint32_t* out, uint64_t half) {
    return (half & 3) == 0 && !(((uintptr_t)evals | (uintptr_t)out) & 15);
}

// FRI fold, structured points; 4 outputs per thread through 16-byte accesses when the layer allows.
// NT: non-temporal accesses for layers far larger than the Infinity Cache (read once, written once).
// COMMIT: the same sweep also hashes the leaves of the FOLDED layer's Merkle tree (src/fibonacci.rs:233-241: the layer is
// committed right after it is folded), so the new layer is produced and leaf-hashed in one pass over the old one:
// leaves[i] = SHA256(0x00 || salt_i || out[i]) (salts == nullptr: the unsalted final-layer form).
template <bool NT, bool COMMIT = false>
__global__ void __launch_bounds__(256) fri_fold_kernel(const FoldArgs f, const uint4* __restrict__ salts = nullptr, Digest* __restrict__ leaves = nullptr) {
    const uint64_t half = f.half;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // COMMIT: one output and one leaf hash per thread (a SHA-256 compression is ~1 500 instructions against ~20 for the fold:
    // the sweep is hash-bound, so it is kept as wide as the separate leaf kernel)
    if (!COMMIT && fold_quads(f.evals, f.out, half)) {
        const uint4* ea = reinterpret_cast<const uint4*>(f.evals);
        const uint4* eb = reinterpret_cast<const uint4*>(f.evals + half);
        uint4* o = reinterpret_cast<uint4*>(f.out);
        for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < half / 4; q += stride) {
            uint4 a, b;
            if constexpr (NT) {
                const u32x4 va = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ea + q));
                const u32x4 vb = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(eb + q));
                a = make_uint4(va.x, va.y, va.z, va.w);
                b = make_uint4(vb.x, vb.y, vb.z, vb.w);
            } else {
                a = ea[q];
                b = eb[q];
            }
            uint4 r;
            r.x = fold_one(f, 4 * q + 0, a.x, b.x);
            r.y = fold_one(f, 4 * q + 1, a.y, b.y);
            r.z = fold_one(f, 4 * q + 2, a.z, b.z);
            r.w = fold_one(f, 4 * q + 3, a.w, b.w);
            if constexpr (NT) {
                u32x4 vr = {r.x, r.y, r.z, r.w};
                __builtin_nontemporal_store(vr, reinterpret_cast<u32x4*>(o + q));
            } else {
                o[q] = r;
            }
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += stride) {
            const uint32_t r = fold_one(f, i, f.evals[i], f.evals[i + half]);
            f.out[i] = r;
            if constexpr (COMMIT) {
                if (salts) {
                    const uint4 sv = salts[i];
                    const uint32_t sw[4] = {sv.x, sv.y, sv.z, sv.w};
                    leaves[i] = merkle_leaf(r, sw);
                } else {
                    leaves[i] = merkle_leaf(r, nullptr);
                }
            }
        }
    }
}

// The plain fold of a large layer as a shaped stream (round 3): T-thread workgroups, U independent 16-byte load pairs in flight per
// lane, a workgroup covering U * T consecutive quads per iteration -- the shape in which a copy reaches the box's 6.2 TB/s
// (profiles/r03_copyceiling.txt: 1024 threads x 4 in flight) -- and one table lookup per four outputs (fold_quad).
template <bool NT, int T, int U>
__global__ void __launch_bounds__(T) fri_fold_stream_kernel(const FoldArgs f) {
    const uint64_t quads = f.half / 4;
    const uint4* ea = reinterpret_cast<const uint4*>(f.evals);
    const uint4* eb = reinterpret_cast<const uint4*>(f.evals + f.half);
    uint4* o = reinterpret_cast<uint4*>(f.out);
    const uint64_t chunk = (uint64_t)U * T;
    for (uint64_t c0 = (uint64_t)blockIdx.x * chunk; c0 < quads; c0 += (uint64_t)gridDim.x * chunk) {
        uint4 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t q = c0 + (uint64_t)u * T + threadIdx.x;
            if (q < quads) {
                if constexpr (NT) {
                    const u32x4 va = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ea + q));
                    const u32x4 vb = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(eb + q));
                    a[u] = make_uint4(va.x, va.y, va.z, va.w);
                    b[u] = make_uint4(vb.x, vb.y, vb.z, vb.w);
                } else {
                    a[u] = ea[q];
                    b[u] = eb[q];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t q = c0 + (uint64_t)u * T + threadIdx.x;
            if (q < quads) {
                const uint32_t av[4] = {a[u].x, a[u].y, a[u].z, a[u].w}, bv[4] = {b[u].x, b[u].y, b[u].z, b[u].w};
                uint32_t r[4];
                fold_quad(f, 4 * q, av, bv, r);
                if constexpr (NT) {
                    u32x4 vr = {r[0], r[1], r[2], r[3]};
                    __builtin_nontemporal_store(vr, reinterpret_cast<u32x4*>(o + q));
                } else {
                    o[q] = make_uint4(r[0], r[1], r[2], r[3]);
                }
            }
        }
    }
}

// ---- salts (prover_kernels.hpp: chacha20_block) ----
struct ChaChaArgs {
    uint32_t key[8];
    uint32_t nonce[3];
    uint64_t blocks;
    uint4* out;
};
__global__ void __launch_bounds__(256) chacha20_fill_kernel(const ChaChaArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.blocks; b += stride) {
        uint32_t o[16];
        chacha20_block(a.key, (uint32_t)b, a.nonce, o);
#pragma unroll
        for (int q = 0; q < 4; ++q) a.out[4 * b + q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
}

// ---- pointwise prover steps (prover_kernels.hpp) ----
// constraint + quotient: 4 consecutive points per thread (16-byte accesses; the three trace reads of a point are B and 2B
// words apart, B = blow-up, so they stay 16-byte aligned when B >= 4); 1 / Z_H per residue class in LDS
__global__ void __launch_bounds__(256) fib_quotient_kernel(const QuotientArgs a) {
    __shared__ uint32_t zh_inv[1024];
    const uint32_t B = 1u << a.log_blowup;
    for (uint32_t t = threadIdx.x; t < B; t += blockDim.x) zh_inv[t] = quotient_zh_inv(a, t);
    __syncthreads();
    const uint64_t N = (uint64_t)1 << a.log_N, mask = N - 1;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    if (a.log_blowup >= 2 && a.log_N >= 2 && !(((uintptr_t)a.trace | (uintptr_t)a.c_out | (uintptr_t)a.q_out) & 15)) {
        const uint4* tr = reinterpret_cast<const uint4*>(a.trace);
        for (uint64_t qd = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; qd < N / 4; qd += stride) {
            const uint64_t i = 4 * qd;
            const uint4 v0 = tr[qd], v1 = tr[((i + B) & mask) >> 2], v2 = tr[((i + 2 * B) & mask) >> 2];
            const uint32_t t0[4] = {v0.x, v0.y, v0.z, v0.w}, t1[4] = {v1.x, v1.y, v1.z, v1.w}, t2[4] = {v2.x, v2.y, v2.z, v2.w};
            uint32_t c[4], qv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) quotient_one(a, i + j, t0[j], t1[j], t2[j], zh_inv[(i + j) & (B - 1)], c[j], qv[j]);
            if (a.c_out) reinterpret_cast<uint4*>(a.c_out)[qd] = make_uint4(c[0], c[1], c[2], c[3]);
            reinterpret_cast<uint4*>(a.q_out)[qd] = make_uint4(qv[0], qv[1], qv[2], qv[3]);
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
            uint32_t c, qv;
            quotient_one(a, i, a.trace[i], a.trace[(i + B) & mask], a.trace[(i + 2 * B) & mask], zh_inv[i & (B - 1)], c, qv);
            if (a.c_out) a.c_out[i] = c;
            a.q_out[i] = qv;
        }
    }
}

// DEEP layer: 8 consecutive points per thread share one inversion
__global__ void __launch_bounds__(256) fib_deep_kernel(const DeepArgs a) {
    constexpr int K = 8;
    const uint64_t N = (uint64_t)1 << a.log_N, mask = N - 1, B = (uint64_t)1 << a.log_blowup;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    if (a.log_N >= 3) {
        for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < N / K; g += stride) {
            const uint64_t i0 = g * K;
            uint32_t t0[K], t1[K], t2[K], qv[K], out[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {   // consecutive addresses: the compiler merges them into 16-byte loads when B is a multiple of 4
                t0[j] = a.trace[i0 + j];
                t1[j] = a.trace[(i0 + j + B) & mask];
                t2[j] = a.trace[(i0 + j + 2 * B) & mask];
                qv[j] = a.quot[i0 + j];
            }
            deep_group<K>(a, i0, t0, t1, t2, qv, out);
#pragma unroll
            for (int j = 0; j < K; ++j) a.out[i0 + j] = out[j];
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
            const uint32_t t0[1] = {a.trace[i]}, t1[1] = {a.trace[(i + B) & mask]}, t2[1] = {a.trace[(i + 2 * B) & mask]}, qv[1] = {a.quot[i]};
            uint32_t out[1];
            deep_group<1>(a, i, t0, t1, t2, qv, out);
            a.out[i] = out[0];
        }
    }
}

// block-wide sum mod p through LDS (256 threads)
__device__ __forceinline__ uint32_t block_sum_mod(uint32_t v, uint32_t* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] = bb_add(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    const uint32_t r = red[0];
    __syncthreads();
    return r;
}
// polynomial evaluation, stage 1: every block reduces one chunk of POLY_CHUNK coefficients for all points
__global__ void __launch_bounds__(256) poly_eval_partial_kernel(const PolyEvalArgs a) {
    __shared__ uint32_t red[256];
    const uint64_t base = (uint64_t)blockIdx.x * POLY_CHUNK + (uint64_t)threadIdx.x * POLY_PER_THREAD;
    uint32_t c[POLY_PER_THREAD];
#pragma unroll
    for (uint32_t j = 0; j < POLY_PER_THREAD; ++j) c[j] = base + j < a.ncoeffs ? a.coeffs[base + j] : 0u;
    for (uint32_t p = 0; p < a.npoints; ++p) {
        const uint32_t sum = block_sum_mod(poly_thread_term(a, p, c, threadIdx.x), red);
        if (threadIdx.x == 0) a.partial[(uint64_t)blockIdx.x * a.npoints + p] = sum;
    }
}
// stage 2 (one block): out[p] = sum_b partial[b][p] * (z^POLY_CHUNK)^b
__global__ void __launch_bounds__(256) poly_eval_final_kernel(const PolyEvalArgs a) {
    __shared__ uint32_t red[256];
    for (uint32_t p = 0; p < a.npoints; ++p) {
        uint32_t acc = 0;
        for (uint32_t b = threadIdx.x; b < a.nblocks; b += blockDim.x)
            acc = bb_add(acc, mont_mul(a.partial[(uint64_t)b * a.npoints + p], mont_pow(a.zchunkR[p], b)));
        const uint32_t sum = block_sum_mod(acc, red);
        if (threadIdx.x == 0) a.out[p] = sum;
    }
}

// the batched form: grid (chunk, column) -- columns beyond the grid's y extent are taken in further rounds
__global__ void __launch_bounds__(256) poly_eval_batch_partial_kernel(const PolyBatchArgs a) {
    __shared__ uint32_t red[256];
    for (uint32_t col = blockIdx.y; col < a.batch; col += gridDim.y) {
        uint32_t c[POLY_PER_THREAD];
        poly_batch_load(a, col, blockIdx.x, threadIdx.x, c);
        for (uint32_t p = 0; p < a.e.npoints; ++p) {
            const uint32_t sum = block_sum_mod(poly_thread_term(a.e, p, c, threadIdx.x), red);
            if (threadIdx.x == 0) a.e.partial[poly_batch_partial_index(a, col, blockIdx.x, p)] = sum;
        }
    }
}
// one block per column
__global__ void __launch_bounds__(256) poly_eval_batch_final_kernel(const PolyBatchArgs a) {
    __shared__ uint32_t red[256];
    for (uint32_t col = blockIdx.x; col < a.batch; col += gridDim.x)
        for (uint32_t p = 0; p < a.e.npoints; ++p) {
            const uint32_t sum = block_sum_mod(poly_batch_final_thread(a, col, p, threadIdx.x, blockDim.x), red);
            if (threadIdx.x == 0) a.e.out[(uint64_t)col * a.e.npoints + p] = sum;
        }
}

// DEEP combination of a column-major matrix: one group of 8 consecutive points per thread (no grid-stride loop: every read of
// the term table then precedes the thread's only stores, so the table is fetched by scalar loads); single points below N = 8
__device__ __forceinline__ void deep_combine_body(const DeepCombineArgs& a, const DeepTerm* terms) {
    constexpr int K = 8;
    const uint64_t N = (uint64_t)1 << a.log_N;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.log_N >= 3) {
        if (g >= N / K) return;
        const uint64_t i0 = g * K;
        uint32_t d[K];
        deep_combine_group<K>(a, terms, i0, d);
        uint4* o = reinterpret_cast<uint4*>(a.out + i0);
        if (!((uintptr_t)a.out & 15)) {
            if (a.accumulate) {
                const uint4 p0 = o[0], p1 = o[1];
                const uint32_t prev[K] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
                for (int j = 0; j < K; ++j) d[j] = bb_add(prev[j], d[j]);
            }
            o[0] = make_uint4(d[0], d[1], d[2], d[3]);
            o[1] = make_uint4(d[4], d[5], d[6], d[7]);
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) a.out[i0 + j] = a.accumulate ? bb_add(a.out[i0 + j], d[j]) : d[j];
        }
    } else if (g < N) {
        uint32_t d[1];
        deep_combine_group<1>(a, terms, g, d);
        a.out[g] = a.accumulate ? bb_add(a.out[g], d[0]) : d[0];
    }
}
// the table in device memory (any length) ...
__global__ void __launch_bounds__(256) deep_combine_kernel(const DeepCombineArgs a, const DeepTerm* __restrict__ terms) { deep_combine_body(a, terms); }
// ... or, up to DEEP_INLINE_TERMS entries, inside the kernel arguments: no copy ahead of the launch, and the call can be captured
constexpr uint32_t DEEP_INLINE_TERMS = 64;
struct DeepInlineTerms { DeepTerm t[DEEP_INLINE_TERMS]; };
__global__ void __launch_bounds__(256) deep_combine_inline_kernel(const DeepCombineArgs a, const DeepInlineTerms in) { deep_combine_body(a, in.t); }

// The same under Ext challenges (include/toyni_hip.h 3h): one group of 4 consecutive points per thread -- four Ext elements, four
// 16-byte stores (the output is 16-byte aligned by contract) -- and single points below N = 4.  No grid-stride loop, as above.
__device__ __forceinline__ void deep_combine_ext_body(const DeepExtArgs& a, const DeepExtTerm* terms) {
    constexpr int K = 4;
    const uint64_t N = (uint64_t)1 << a.log_N;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.log_N >= 2) {
        if (g >= N / K) return;
        uint32_t d[K][4];
        deep_combine_ext_group<K>(a, terms, g * K, d);
        uint4* o = reinterpret_cast<uint4*>(a.out) + g * K;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (a.accumulate) {
                const uint4 p = o[j];
                o[j] = make_uint4(bb_add(p.x, d[j][0]), bb_add(p.y, d[j][1]), bb_add(p.z, d[j][2]), bb_add(p.w, d[j][3]));
            } else {
                o[j] = make_uint4(d[j][0], d[j][1], d[j][2], d[j][3]);
            }
        }
    } else if (g < N) {
        uint32_t d[1][4];
        deep_combine_ext_group<1>(a, terms, g, d);
        uint4* o = reinterpret_cast<uint4*>(a.out) + g;
        const uint4 p = a.accumulate ? o[0] : make_uint4(0u, 0u, 0u, 0u);
        o[0] = make_uint4(bb_add(p.x, d[0][0]), bb_add(p.y, d[0][1]), bb_add(p.z, d[0][2]), bb_add(p.w, d[0][3]));
    }
}
__global__ void __launch_bounds__(256) deep_combine_ext_kernel(const DeepExtArgs a, const DeepExtTerm* __restrict__ terms) { deep_combine_ext_body(a, terms); }
// up to DEEP_EXT_INLINE_TERMS entries of 32 bytes inside the kernel arguments (2 KiB): capturable, no copy ahead of the launch
constexpr uint32_t DEEP_EXT_INLINE_TERMS = 64;
struct DeepExtInlineTerms { DeepExtTerm t[DEEP_EXT_INLINE_TERMS]; };
__global__ void __launch_bounds__(256) deep_combine_ext_inline_kernel(const DeepExtArgs a, const DeepExtInlineTerms in) { deep_combine_ext_body(a, in.t); }

// Polynomial evaluation at Ext points, the two stages of the batched form above; block_sum_mod runs once per coordinate
__global__ void __launch_bounds__(256) poly_eval_ext_batch_partial_kernel(const PolyExtArgs a) {
    __shared__ uint32_t red[256];
    for (uint32_t col = blockIdx.y; col < a.batch; col += gridDim.y) {
        uint32_t c[POLY_PER_THREAD];
        poly_ext_load(a, col, blockIdx.x, threadIdx.x, c);
        for (uint32_t p = 0; p < a.npoints; ++p) {
            const Ext4 v = poly_ext_thread_term(a, p, c, threadIdx.x);
            uint32_t* dst = a.partial + poly_ext_partial_index(a, col, blockIdx.x, p);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t sum = block_sum_mod(v.c[k], red);
                if (threadIdx.x == 0) dst[k] = sum;
            }
        }
    }
}
// one block per column
__global__ void __launch_bounds__(256) poly_eval_ext_batch_final_kernel(const PolyExtArgs a) {
    __shared__ uint32_t red[256];
    for (uint32_t col = blockIdx.x; col < a.batch; col += gridDim.x)
        for (uint32_t p = 0; p < a.npoints; ++p) {
            const Ext4 v = poly_ext_final_thread(a, col, p, threadIdx.x);
            uint32_t* dst = a.out + ((uint64_t)col * a.npoints + p) * 4u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t sum = block_sum_mod(v.c[k], red);
                if (threadIdx.x == 0) dst[k] = sum;
            }
        }
}

// Constraint program of an AIR (prover_kernels.hpp): one group of 4 consecutive points per thread, single points below N = 4.  No
// grid-stride loop: every read of the program and of the weights precedes the thread's only global stores, so both are fetched
// by scalar loads.  Dynamic LDS: [nregs][threads] slots of 16 bytes (the register file, sized from the program), then 1 / Z_H of
// the B residue classes when they fit (a.zh_lds).
#ifndef TOYNI_KERNEL_TEXT_ONLY
extern __shared__ __align__(16) uint32_t air_lds[];
#else
extern __align__(16) uint32_t air_lds[];   // (`extern static` is not C++: the including translation unit defines the array)
#endif
__device__ __forceinline__ void air_quotient_body(const AirArgs& a, const uint32_t* weights) {
    constexpr int K = 4;
    const uint32_t B = 1u << a.log_blowup;
    uint32_t* zh_lds = air_lds + a.nregs * blockDim.x * K;
    if (a.zh_lds) {
        for (uint32_t t = threadIdx.x; t < B; t += blockDim.x) zh_lds[t] = zh_inv_class(a.shift_nR, a.wBR, t);
        __syncthreads();
    }
    const uint64_t N = (uint64_t)1 << a.log_N;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.log_N >= 2) {
        if (g >= N / K) return;
        const uint64_t i0 = g * K;
        uint32_t zhR[K], c[K], q[K];
        if (a.zh_lds) {
#pragma unroll
            for (int j = 0; j < K; ++j) zhR[j] = zh_lds[(i0 + j) & (B - 1)];
        } else if (a.divides) {
            air_zh_inverses<K>(a, i0, zhR);
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) zhR[j] = 0u;
        }
        air_eval_group<K>(a, weights, air_lds + threadIdx.x * K, blockDim.x * K, i0, zhR, c, q);
        uint32_t* outs[2] = {a.c_out, a.q_out};
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            uint32_t* dst = outs[o];
            if (!dst) continue;
            uint32_t (&v)[K] = o ? q : c;
            if (!((uintptr_t)dst & 15)) {
                uint4* d4 = reinterpret_cast<uint4*>(dst + i0);
                if (a.accumulate) {
                    const uint4 p = *d4;
                    v[0] = bb_add(p.x, v[0]); v[1] = bb_add(p.y, v[1]); v[2] = bb_add(p.z, v[2]); v[3] = bb_add(p.w, v[3]);
                }
                *d4 = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) dst[i0 + j] = a.accumulate ? bb_add(dst[i0 + j], v[j]) : v[j];
            }
        }
    } else if (g < N) {
        uint32_t zhR[1] = {0u}, c[1], q[1];
        if (a.zh_lds) zhR[0] = zh_lds[g & (B - 1)];
        else if (a.divides) air_zh_inverses<1>(a, g, zhR);
        air_eval_group<1>(a, weights, air_lds + threadIdx.x, blockDim.x, g, zhR, c, q);
        if (a.c_out) a.c_out[g] = a.accumulate ? bb_add(a.c_out[g], c[0]) : c[0];
        a.q_out[g] = a.accumulate ? bb_add(a.q_out[g], q[0]) : q[0];
    }
}
// the weights in device memory (any number) ...
__global__ void __launch_bounds__(256) air_quotient_kernel(const AirArgs a, const uint32_t* __restrict__ weights) { air_quotient_body(a, weights); }
// ... or, up to AIR_INLINE_WEIGHTS of them, inside the kernel arguments (as deep_combine_inline_kernel)
struct AirInlineWeights { uint32_t w[AIR_INLINE_WEIGHTS]; };
__global__ void __launch_bounds__(256) air_quotient_inline_kernel(const AirArgs a, const AirInlineWeights in) { air_quotient_body(a, in.w); }

// The same programs under Ext weights (include/toyni_hip.h 3k): the launch shape, the LDS layout and the 1 / Z_H classes of
// air_quotient_body, one interpretation per point with four accumulators (air_eval_group_ext), four coordinate columns out.
// a.c_out / a.q_out are the first of four columns each, out_stride words apart.
__device__ __forceinline__ void air_quotient_ext_body(const AirArgs& a, uint64_t out_stride, const uint32_t* weights4) {
    constexpr int K = 4;
    const uint32_t B = 1u << a.log_blowup;
    uint32_t* zh_lds = air_lds + a.nregs * blockDim.x * K;
    if (a.zh_lds) {
        for (uint32_t t = threadIdx.x; t < B; t += blockDim.x) zh_lds[t] = zh_inv_class(a.shift_nR, a.wBR, t);
        __syncthreads();
    }
    const uint64_t N = (uint64_t)1 << a.log_N;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.log_N >= 2) {
        if (g >= N / K) return;
        const uint64_t i0 = g * K;
        uint32_t zhR[K], c[4][K], q[4][K];
        if (a.zh_lds) {
#pragma unroll
            for (int j = 0; j < K; ++j) zhR[j] = zh_lds[(i0 + j) & (B - 1)];
        } else if (a.divides) {
            air_zh_inverses<K>(a, i0, zhR);
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) zhR[j] = 0u;
        }
        air_eval_group_ext<K>(a, weights4, air_lds + threadIdx.x * K, blockDim.x * K, i0, zhR, c, q);
        air_ext_store<K>(a.c_out, out_stride, i0, a.accumulate, c);
        air_ext_store<K>(a.q_out, out_stride, i0, a.accumulate, q);
    } else if (g < N) {
        uint32_t zhR[1] = {0u}, c[4][1], q[4][1];
        if (a.zh_lds) zhR[0] = zh_lds[g & (B - 1)];
        else if (a.divides) air_zh_inverses<1>(a, g, zhR);
        air_eval_group_ext<1>(a, weights4, air_lds + threadIdx.x, blockDim.x, g, zhR, c, q);
        air_ext_store<1>(a.c_out, out_stride, g, a.accumulate, c);
        air_ext_store<1>(a.q_out, out_stride, g, a.accumulate, q);
    }
}
__global__ void __launch_bounds__(256) air_quotient_ext_kernel(const AirArgs a, const uint64_t out_stride, const uint32_t* __restrict__ weights4) {
    air_quotient_ext_body(a, out_stride, weights4);
}
// up to AIR_EXT_INLINE_WEIGHTS Ext weights inside the kernel arguments
struct AirExtInlineWeights { uint32_t w[4 * AIR_EXT_INLINE_WEIGHTS]; };
__global__ void __launch_bounds__(256) air_quotient_ext_inline_kernel(const AirArgs a, const uint64_t out_stride, const AirExtInlineWeights in) {
    air_quotient_ext_body(a, out_stride, in.w);
}

// Accumulator columns (prover_kernels.hpp, include/toyni_hip.h 3g).  Every workgroup is SCAN_THREADS threads, every thread owns
// SCAN_GROUP consecutive elements.  The workgroup-wide scan: thread-serial over the group (the caller), log2(64) cross-lane steps
// inside each wave, the waves' totals through LDS.  Every thread of the workgroup reaches both barriers.
template <int OP>
__device__ __forceinline__ uint32_t scan_wave_inclusive(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t delta = 1; delta < SCAN_WAVE; delta <<= 1) v = scan_wave_step<OP>(v, scan_lane_up(v, delta), lane, delta);
    return v;
}
// what the threads below this one add up to, and in `total` the whole workgroup's; wave_tot: SCAN_THREADS / 64 words of LDS
template <int OP>
__device__ __forceinline__ uint32_t scan_block_exclusive(uint32_t v, uint32_t* wave_tot, uint32_t& total) {
    constexpr int NW = SCAN_THREADS / SCAN_WAVE;
    const uint32_t lane = threadIdx.x & (SCAN_WAVE - 1), wave = threadIdx.x / SCAN_WAVE;
    const uint32_t inc = scan_wave_inclusive<OP>(v, lane);
    if (lane == SCAN_WAVE - 1) wave_tot[wave] = inc;
    __syncthreads();
    const uint32_t up = scan_lane_up(inc, 1);
    const uint32_t pre = scan_waves_below<OP, NW>(wave_tot, wave, total);
    __syncthreads();   // wave_tot may be written again
    return lane ? scan_combine<OP>(pre, up) : pre;
}
// step 1, grid (tile, column): one aggregate and one zero count per tile
template <int OP>
__global__ void __launch_bounds__(SCAN_THREADS) column_scan_aggregate_kernel(const ScanArgs a) {
    __shared__ uint32_t wave_tot[SCAN_THREADS / SCAN_WAVE];
    const uint32_t col = blockIdx.y, tile = blockIdx.x;
    const uint64_t i0 = (uint64_t)tile * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_GROUP;
    uint32_t t[SCAN_GROUP], ex[SCAN_GROUP], total, ztotal;
    const uint32_t zeros = scan_group_terms<OP, SCAN_GROUP>(a.num ? a.num + col * a.num_stride : nullptr, a.den ? a.den + col * a.den_stride : nullptr,
                                                            i0, a.n, t);
    (void)scan_block_exclusive<OP>(scan_thread_serial<OP, SCAN_GROUP>(t, ex), wave_tot, total);
    (void)scan_block_exclusive<SCAN_COUNT>(zeros, wave_tot, ztotal);
    if (threadIdx.x == 0) {
        scan_tile_aggregates(a, col)[tile] = total;
        scan_tile_zeros(a, col)[tile] = ztotal;
    }
}
// step 2, one workgroup per column: the exclusive scan of the column's aggregates, seeded with init, in rounds of SCAN_TILE; the totals
template <int OP>
__global__ void __launch_bounds__(SCAN_THREADS) column_scan_prefix_kernel(const ScanArgs a, const ScanInit in) {
    __shared__ uint32_t wave_tot[SCAN_THREADS / SCAN_WAVE];
    const uint32_t col = blockIdx.x;
    uint32_t* agg = scan_tile_aggregates(a, col);
    uint32_t carry = in.v[col];
    for (uint32_t base = 0; base < a.ntiles; base += SCAN_TILE) {
        const uint64_t i0 = (uint64_t)base + threadIdx.x * SCAN_GROUP;
        uint32_t t[SCAN_GROUP], ex[SCAN_GROUP], total;
        scan_group_load<SCAN_GROUP>(agg, i0, a.ntiles, scan_identity<OP>(), t);
        const uint32_t pre = scan_block_exclusive<OP>(scan_thread_serial<OP, SCAN_GROUP>(t, ex), wave_tot, total);
        const uint32_t mine = scan_combine<OP>(carry, pre);
#pragma unroll
        for (int j = 0; j < (int)SCAN_GROUP; ++j) t[j] = scan_combine<OP>(mine, ex[j]);
        scan_group_store<SCAN_GROUP>(agg, i0, a.ntiles, t);
        carry = scan_combine<OP>(carry, total);
    }
    const uint32_t* zc = scan_tile_zeros(a, col);
    uint32_t zeros = 0, ztotal;
    for (uint32_t k = threadIdx.x; k < a.ntiles; k += SCAN_THREADS) zeros += zc[k];
    (void)scan_block_exclusive<SCAN_COUNT>(zeros, wave_tot, ztotal);
    if (threadIdx.x == 0 && a.totals) {
        a.totals[2 * col] = scan_to_plain<OP>(carry);
        a.totals[2 * col + 1] = ztotal;
    }
}
// step 3, grid (tile, column): the terms again, the scan inside the tile on top of the tile's prefix.  With a.single the grid is the
// columns alone (n <= one tile): the prefix is init and the totals are written here.
template <int OP>
__global__ void __launch_bounds__(SCAN_THREADS) column_scan_apply_kernel(const ScanArgs a, const ScanInit in) {
    __shared__ uint32_t wave_tot[SCAN_THREADS / SCAN_WAVE];
    const uint32_t col = blockIdx.y, tile = blockIdx.x;
    const uint64_t i0 = (uint64_t)tile * SCAN_TILE + (uint64_t)threadIdx.x * SCAN_GROUP;
    uint32_t t[SCAN_GROUP], ex[SCAN_GROUP], total;
    const uint32_t zeros = scan_group_terms<OP, SCAN_GROUP>(a.num ? a.num + col * a.num_stride : nullptr, a.den ? a.den + col * a.den_stride : nullptr,
                                                            i0, a.n, t);
    const uint32_t pre = scan_block_exclusive<OP>(scan_thread_serial<OP, SCAN_GROUP>(t, ex), wave_tot, total);
    const uint32_t seed = a.single ? in.v[col] : TOYNI_UNIFORM(scan_tile_aggregates(a, col)[tile]);
    scan_group_finish<OP, SCAN_GROUP>(scan_combine<OP>(seed, pre), ex, t);
    scan_group_store<SCAN_GROUP>(a.out + col * a.out_stride, i0, a.n, t);
    if (a.single) {
        uint32_t ztotal;
        (void)scan_block_exclusive<SCAN_COUNT>(zeros, wave_tot, ztotal);
        if (threadIdx.x == 0 && a.totals) {
            a.totals[2 * col] = scan_to_plain<OP>(scan_combine<OP>(seed, total));
            a.totals[2 * col + 1] = ztotal;
        }
    }
}
// out[i] = in[i]^-1 (0 for 0): the term-forming group body alone.  zero_count (may be null) was cleared ahead of the launch.
__global__ void __launch_bounds__(SCAN_THREADS) batch_inverse_kernel(const uint32_t* in, uint32_t* out, uint64_t count, uint32_t* zero_count) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * SCAN_THREADS + threadIdx.x) * SCAN_GROUP;
    uint32_t t[SCAN_GROUP];
    const uint32_t zeros = scan_group_terms<SCAN_SUM, SCAN_GROUP>(nullptr, in, i0, count, t);
    scan_group_store<SCAN_GROUP>(out, i0, count, t);
    if (zero_count) {
        const uint32_t lane = threadIdx.x & (SCAN_WAVE - 1);
        const uint32_t wave_zeros = scan_wave_inclusive<SCAN_COUNT>(zeros, lane);
        if (lane == SCAN_WAVE - 1 && wave_zeros) atomicAdd(zero_count, wave_zeros);
    }
}

// Accumulator columns under an Ext challenge (prover_kernels.hpp, include/toyni_hip.h 3i): the three launches above with Ext values.
// Every workgroup is EXT_ACCUM_THREADS threads, every thread owns EXT_ACCUM_GROUP consecutive elements; the cross-lane step moves the
// four words of a value, the waves' totals go through 16 bytes of LDS per wave.  Every thread of the workgroup reaches both barriers.
template <int OP>
__device__ __forceinline__ Ext4 ext_accum_wave_inclusive(Ext4 v, uint32_t lane) {
#pragma unroll
    for (uint32_t delta = 1; delta < SCAN_WAVE; delta <<= 1) {
        Ext4 below;
#pragma unroll
        for (int k = 0; k < 4; ++k) below.c[k] = scan_lane_up(v.c[k], delta);
        if (lane >= delta) v = ext_accum_combine<OP>(below, v);
    }
    return v;
}
// what the threads below this one combine to, and in `total` the whole workgroup's; wave_tot: EXT_ACCUM_THREADS / 64 values of LDS
template <int OP>
__device__ __forceinline__ Ext4 ext_accum_block_exclusive(const Ext4& v, Ext4* wave_tot, Ext4& total) {
    constexpr int NW = EXT_ACCUM_THREADS / SCAN_WAVE;
    const uint32_t lane = threadIdx.x & (SCAN_WAVE - 1), wave = threadIdx.x / SCAN_WAVE;
    const Ext4 inc = ext_accum_wave_inclusive<OP>(v, lane);
    if (lane == SCAN_WAVE - 1) wave_tot[wave] = inc;
    __syncthreads();
    Ext4 up;
#pragma unroll
    for (int k = 0; k < 4; ++k) up.c[k] = scan_lane_up(inc.c[k], 1);
    const Ext4 pre = ext_accum_waves_below<OP, NW>(wave_tot, wave, total);
    __syncthreads();   // wave_tot may be written again
    return lane ? ext_accum_combine<OP>(pre, up) : pre;
}
static_assert(EXT_ACCUM_THREADS == SCAN_THREADS, "the zero counts go through scan_block_exclusive<SCAN_COUNT>");
// step 1, grid (tile, column): one aggregate and one zero count per tile
template <int OP>
__device__ __forceinline__ void ext_accum_aggregate_body(const ExtAccumArgs& a, Ext4* wave_tot, uint32_t* wave_zeros) {
    const uint32_t col = blockIdx.y, tile = blockIdx.x;
    const uint64_t i0 = (uint64_t)tile * EXT_ACCUM_TILE + (uint64_t)threadIdx.x * EXT_ACCUM_GROUP;
    Ext4 t[EXT_ACCUM_GROUP], ex[EXT_ACCUM_GROUP], total;
    uint32_t ztotal;
    const uint32_t zeros = ext_accum_group_terms<OP, EXT_ACCUM_GROUP>(a, col, i0, a.n, t);
    (void)ext_accum_block_exclusive<OP>(ext_accum_thread_serial<OP, EXT_ACCUM_GROUP>(t, ex), wave_tot, total);
    (void)scan_block_exclusive<SCAN_COUNT>(zeros, wave_zeros, ztotal);
    if (threadIdx.x == 0) {
        uint32_t* agg = ext_accum_tile_aggregates(a, col);
#pragma unroll
        for (int k = 0; k < 4; ++k) agg[(uint64_t)k * a.ntiles + tile] = total.c[k];
        ext_accum_tile_zeros(a, col)[tile] = ztotal;
    }
}
template <int OP>
__global__ void __launch_bounds__(EXT_ACCUM_THREADS) ext_accum_aggregate_kernel(const ExtAccumArgs a) {
    __shared__ Ext4 wave_tot[EXT_ACCUM_THREADS / SCAN_WAVE];
    __shared__ uint32_t wave_zeros[EXT_ACCUM_THREADS / SCAN_WAVE];
    ext_accum_aggregate_body<OP>(a, wave_tot, wave_zeros);
}
// step 2, one workgroup per column: the exclusive scan of the column's aggregates, seeded with init, in rounds of EXT_ACCUM_TILE; the totals
template <int OP>
__global__ void __launch_bounds__(EXT_ACCUM_THREADS) ext_accum_prefix_kernel(const ExtAccumArgs a, const ExtAccumSeeds in) {
    __shared__ Ext4 wave_tot[EXT_ACCUM_THREADS / SCAN_WAVE];
    __shared__ uint32_t wave_zeros[EXT_ACCUM_THREADS / SCAN_WAVE];
    const uint32_t col = blockIdx.x;
    uint32_t* agg = ext_accum_tile_aggregates(a, col);
    Ext4 carry = {{in.v[col][0], in.v[col][1], in.v[col][2], in.v[col][3]}};
    for (uint32_t base = 0; base < a.ntiles; base += EXT_ACCUM_TILE) {
        const uint64_t i0 = (uint64_t)base + threadIdx.x * EXT_ACCUM_GROUP;
        Ext4 t[EXT_ACCUM_GROUP], ex[EXT_ACCUM_GROUP], total;
        ext_column_group_load<EXT_ACCUM_GROUP>(agg, a.ntiles, i0, a.ntiles, t);
#pragma unroll
        for (int j = 0; j < (int)EXT_ACCUM_GROUP; ++j)
            if (i0 + (uint64_t)j >= a.ntiles) t[j] = ext_accum_identity<OP>();
        const Ext4 pre = ext_accum_block_exclusive<OP>(ext_accum_thread_serial<OP, EXT_ACCUM_GROUP>(t, ex), wave_tot, total);
        const Ext4 mine = ext_accum_combine<OP>(carry, pre);
#pragma unroll
        for (int j = 0; j < (int)EXT_ACCUM_GROUP; ++j) t[j] = ext_accum_combine<OP>(mine, ex[j]);
        ext_column_group_store<EXT_ACCUM_GROUP>(agg, a.ntiles, i0, a.ntiles, t);
        carry = ext_accum_combine<OP>(carry, total);
    }
    const uint32_t* zc = ext_accum_tile_zeros(a, col);
    uint32_t zeros = 0, ztotal;
    for (uint32_t k = threadIdx.x; k < a.ntiles; k += EXT_ACCUM_THREADS) zeros += zc[k];
    (void)scan_block_exclusive<SCAN_COUNT>(zeros, wave_zeros, ztotal);
    if (threadIdx.x == 0 && a.totals) {
        const Ext4 tot = ext_accum_to_plain<OP>(carry);
#pragma unroll
        for (int k = 0; k < 4; ++k) a.totals[8 * col + k] = tot.c[k];
        a.totals[8 * col + 4] = ztotal;
#pragma unroll
        for (int k = 5; k < 8; ++k) a.totals[8 * col + k] = 0u;
    }
}
// step 3, grid (tile, column): the terms again, the scan inside the tile on top of the tile's prefix.  With a.single the grid is the
// columns alone (n <= one tile): the prefix is init and the totals are written here.  In place on a width-4 operand: a thread has read
// all it needs of its own elements before it stores them, and no thread reads another's.
template <int OP>
__device__ __forceinline__ void ext_accum_apply_body(const ExtAccumArgs& a, const ExtAccumSeeds& in, Ext4* wave_tot, uint32_t* wave_zeros) {
    const uint32_t col = blockIdx.y, tile = blockIdx.x;
    const uint64_t i0 = (uint64_t)tile * EXT_ACCUM_TILE + (uint64_t)threadIdx.x * EXT_ACCUM_GROUP;
    Ext4 t[EXT_ACCUM_GROUP], ex[EXT_ACCUM_GROUP], total, seed;
    const uint32_t zeros = ext_accum_group_terms<OP, EXT_ACCUM_GROUP>(a, col, i0, a.n, t);
    const Ext4 pre = ext_accum_block_exclusive<OP>(ext_accum_thread_serial<OP, EXT_ACCUM_GROUP>(t, ex), wave_tot, total);
    const uint32_t* agg = ext_accum_tile_aggregates(a, col);
#pragma unroll
    for (int k = 0; k < 4; ++k) seed.c[k] = a.single ? in.v[col][k] : TOYNI_UNIFORM(agg[(uint64_t)k * a.ntiles + tile]);
    ext_accum_group_finish<OP, EXT_ACCUM_GROUP>(ext_accum_combine<OP>(seed, pre), ex, t);
    ext_column_group_store<EXT_ACCUM_GROUP>(a.out + 4ull * col * a.out_stride, a.out_stride, i0, a.n, t);
    if (a.single) {
        uint32_t ztotal;
        (void)scan_block_exclusive<SCAN_COUNT>(zeros, wave_zeros, ztotal);
        if (threadIdx.x == 0 && a.totals) {
            const Ext4 tot = ext_accum_to_plain<OP>(ext_accum_combine<OP>(seed, total));
#pragma unroll
            for (int k = 0; k < 4; ++k) a.totals[8 * col + k] = tot.c[k];
            a.totals[8 * col + 4] = ztotal;
#pragma unroll
            for (int k = 5; k < 8; ++k) a.totals[8 * col + k] = 0u;
        }
    }
}
template <int OP>
__global__ void __launch_bounds__(EXT_ACCUM_THREADS) ext_accum_apply_kernel(const ExtAccumArgs a, const ExtAccumSeeds in) {
    __shared__ Ext4 wave_tot[EXT_ACCUM_THREADS / SCAN_WAVE];
    __shared__ uint32_t wave_zeros[EXT_ACCUM_THREADS / SCAN_WAVE];
    ext_accum_apply_body<OP>(a, in, wave_tot, wave_zeros);
}
// out[i] = in[i]^-1 (0 for 0) on one Ext column: the tower inversion alone.  zero_count (may be null) was cleared ahead of the launch.
__global__ void __launch_bounds__(EXT_ACCUM_THREADS) ext_invert_columns_kernel(const uint32_t* in, uint64_t in_stride, uint32_t* out,
                                                                               uint64_t out_stride, uint64_t count, uint32_t* zero_count) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * EXT_ACCUM_THREADS + threadIdx.x) * EXT_ACCUM_GROUP;
    const uint32_t zeros = ext_invert_group<EXT_ACCUM_GROUP>(in, in_stride, out, out_stride, i0, count);
    if (zero_count) {
        const uint32_t lane = threadIdx.x & (SCAN_WAVE - 1);
        const uint32_t wave_zeros = scan_wave_inclusive<SCAN_COUNT>(zeros, lane);
        if (lane == SCAN_WAVE - 1 && wave_zeros) atomicAdd(zero_count, wave_zeros);
    }
}

// Merkle openings: one thread per (opening, level) copies the sibling digest; one thread per opening adds salt, value, flags
struct OpenGroup {
    const Digest* levels;
    uint64_t n;
    const uint32_t* values;
    const uint4* salts;
    const uint32_t* indices;
    uint32_t nidx;
    uint8_t* out;
};
__device__ __forceinline__ void merkle_open_group(const OpenGroup& g, uint64_t first, uint64_t stride) {
    const uint32_t depth = merkle_depth(g.n);
    const uint64_t rec = merkle_open_record_bytes(g.n);
    const uint64_t total = (uint64_t)g.nidx * (depth + 1);
    for (uint64_t w = first; w < total; w += stride) {
        const uint32_t k = (uint32_t)(w / (depth + 1)), level = (uint32_t)(w % (depth + 1));
        const uint64_t index = g.indices[k];
        uint8_t* r = g.out + (uint64_t)k * rec;
        if (level < depth) {
            bool is_left;
            const uint64_t row = merkle_sibling_row(g.n, index, level, is_left);
            reinterpret_cast<Digest*>(r)[level] = g.levels[row];       // records are 8-byte aligned, digests are u32 words
            r[(uint64_t)depth * 32u + 24u + level] = is_left ? 1 : 0;
        } else {
            uint32_t* tail = reinterpret_cast<uint32_t*>(r + (uint64_t)depth * 32u);
            uint4 sv = make_uint4(0u, 0u, 0u, 0u);
            if (g.salts) sv = g.salts[index];
            tail[0] = sv.x; tail[1] = sv.y; tail[2] = sv.z; tail[3] = sv.w;
            tail[4] = g.values[index];
            tail[5] = 0u;
            // padding zero, so a record is a function of the tree alone: byte stores, clear of the position bytes
            // [32 depth + 24, 33 depth + 24) that the other threads of this record write
            for (uint64_t b = (uint64_t)depth * 33u + 24u; b < rec; ++b) r[b] = 0;
        }
    }
}
__global__ void __launch_bounds__(256) merkle_open_kernel(const OpenGroup g) {
    merkle_open_group(g, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
}
// Openings of row leaves (include/toyni_hip.h 3d): per opening, one thread per level copies the sibling digest and writes the position
// byte, one writes salt and padding, one per column writes that value's 8 bytes.  Record: depth x 32 | salt 16 | width x 8 | depth
// position bytes, zero-padded to a multiple of 8 -- merkle_open_kernel's record when width = 1.
struct OpenRows {
    const Digest* levels;
    uint64_t n;
    const uint32_t* values;
    uint32_t width;
    int layout;
    uint64_t col_stride;
    const uint4* salts;
    const uint32_t* indices;
    uint32_t nidx;
    uint8_t* out;
};
__global__ void __launch_bounds__(256) merkle_open_rows_kernel(const OpenRows g) {
    const uint32_t depth = merkle_depth(g.n);
    const uint64_t values_at = (uint64_t)depth * 32u + 16u, flags_at = values_at + 8u * (uint64_t)g.width;
    const uint64_t rec = flags_at + ((depth + 7u) & ~7u);
    const uint64_t per = (uint64_t)depth + 1u + g.width, total = (uint64_t)g.nidx * per;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
        const uint32_t k = (uint32_t)(w / per);
        const uint64_t item = w % per;
        const uint64_t index = g.indices[k];
        uint8_t* r = g.out + (uint64_t)k * rec;
        if (item < depth) {
            bool is_left;
            const uint64_t row = merkle_sibling_row(g.n, index, (uint32_t)item, is_left);
            reinterpret_cast<Digest*>(r)[item] = g.levels[row];        // records are 8-byte aligned, digests are u32 words
            r[flags_at + item] = is_left ? 1 : 0;
        } else if (item == depth) {
            uint32_t* tail = reinterpret_cast<uint32_t*>(r + (uint64_t)depth * 32u);
            uint4 sv = make_uint4(0u, 0u, 0u, 0u);
            if (g.salts) sv = g.salts[index];
            tail[0] = sv.x; tail[1] = sv.y; tail[2] = sv.z; tail[3] = sv.w;
            for (uint64_t b = flags_at + depth; b < rec; ++b) r[b] = 0;   // byte stores, clear of the position bytes
        } else {
            const uint64_t c = item - depth - 1u;
            uint32_t* val = reinterpret_cast<uint32_t*>(r + values_at + 8u * c);
            val[0] = g.layout == TOYNI_ROWS_COLUMN_MAJOR ? g.values[c * g.col_stride + index] : g.values[index * g.width + c];
            val[1] = 0u;
        }
    }
}

// every tree of a proof in ONE launch (blockIdx.y = tree): the 19 launches of a 2^16-row proof's query phase were ~5 us each
constexpr uint32_t OPEN_GROUPS_MAX = 32;
struct OpenGroups { OpenGroup g[OPEN_GROUPS_MAX]; };
__global__ void __launch_bounds__(256) merkle_open_groups_kernel(const OpenGroups gs) {
    merkle_open_group(gs.g[blockIdx.y], (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x);
}

// FRI fold, explicit points, 16 outputs per thread and per Fermat inversion (fold_xs_batch<16>), in the shape of fri_fold_stream_kernel:
// a workgroup covers 4 * T consecutive quads per iteration and a thread takes quad tid of each of the four runs of T, so every
// wave access is 1 KiB of consecutive memory (round 3 gave a thread 16 CONSECUTIVE elements: four 16-byte accesses at a 64-byte lane
// stride, 4.4 TB/s at 2^27) -- Montgomery's trick does not care which 16 points share an inversion.  half a multiple of 4; quads
// past the end ride along as the point 1 with zero values and are not stored.  NT: non-temporal accesses for layers far beyond the
// Infinity Cache.
template <bool NT, int T>
__global__ void __launch_bounds__(T) fri_fold_xs16_kernel(const uint32_t* __restrict__ evals, const uint32_t* __restrict__ xs,
                                                           uint32_t* __restrict__ out, uint64_t half, uint32_t beta_half) {
    const uint64_t quads = half / 4;
    const uint4* ea = reinterpret_cast<const uint4*>(evals);
    const uint4* eb = reinterpret_cast<const uint4*>(evals + half);
    const uint4* xp = reinterpret_cast<const uint4*>(xs);
    uint4* o = reinterpret_cast<uint4*>(out);
    const uint64_t chunk = 4u * T;
    auto load = [](const uint4* p) {
        if constexpr (NT) {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
            return make_uint4(v.x, v.y, v.z, v.w);
        } else {
            return *p;
        }
    };
    for (uint64_t c0 = (uint64_t)blockIdx.x * chunk; c0 < quads; c0 += (uint64_t)gridDim.x * chunk) {
        uint32_t x[16], a[16], b[16], r[16];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t q = c0 + (uint64_t)u * T + threadIdx.x;
            uint4 xv = make_uint4(1u, 1u, 1u, 1u), av = make_uint4(0u, 0u, 0u, 0u), bv = av;
            if (q < quads) { xv = load(xp + q); av = load(ea + q); bv = load(eb + q); }
            x[4 * u] = xv.x; x[4 * u + 1] = xv.y; x[4 * u + 2] = xv.z; x[4 * u + 3] = xv.w;
            a[4 * u] = av.x; a[4 * u + 1] = av.y; a[4 * u + 2] = av.z; a[4 * u + 3] = av.w;
            b[4 * u] = bv.x; b[4 * u + 1] = bv.y; b[4 * u + 2] = bv.z; b[4 * u + 3] = bv.w;
        }
        fold_xs_batch<16>(x, a, b, beta_half, r);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t q = c0 + (uint64_t)u * T + threadIdx.x;
            if (q < quads) {
                if constexpr (NT) {
                    u32x4 vr = {r[4 * u], r[4 * u + 1], r[4 * u + 2], r[4 * u + 3]};
                    __builtin_nontemporal_store(vr, reinterpret_cast<u32x4*>(o + q));
                } else {
                    o[q] = make_uint4(r[4 * u], r[4 * u + 1], r[4 * u + 2], r[4 * u + 3]);
                }
            }
        }
    }
}

// FRI fold, explicit points, 4 outputs per thread and inversion (fold_xs_batch<4>): small layers and ragged tails.
// A zero point is kept OUT of the shared product (it would zero the inverses of its three neighbours): batch_inverse_scaled lets it
// ride along as 1 and forces its own inverse to 0 = pow(0, p-2), what BabyBear::inverse would compute without its zero assert
// (src/babybear.rs:111-114); the host forms report TOYNI_E_ZERO_INVERSE instead.
__global__ void __launch_bounds__(256) fri_fold_xs_kernel(const uint32_t* __restrict__ evals, const uint32_t* __restrict__ xs,
                                                           uint32_t* __restrict__ out, uint64_t half, uint32_t beta_half) {
    // a workgroup covers 4 * 256 consecutive elements per iteration, a thread takes element tid of each of the four runs of 256
    // (consecutive lanes touch consecutive words whatever the alignment; the four points behind one inversion need not be neighbours)
    const uint64_t chunk = 4u * 256u;
    for (uint64_t c0 = (uint64_t)blockIdx.x * chunk; c0 < half; c0 += (uint64_t)gridDim.x * chunk) {
        uint32_t x[4], a[4], b[4], r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t i = c0 + (uint64_t)j * 256u + threadIdx.x;
            const bool in = i < half;
            x[j] = in ? xs[i] : 1u;
            a[j] = in ? evals[i] : 0u;
            b[j] = in ? evals[i + half] : 0u;
        }
        fold_xs_batch<4>(x, a, b, beta_half, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t i = c0 + (uint64_t)j * 256u + threadIdx.x;
            if (i < half) out[i] = r[j];
        }
    }
}

// FRI fold over Ext values (src/math/fri.rs:7-25), AoS 4 x u32 per element = one 16-byte access per lane.
// Structured points x_i = x0 * w_m^i: scale_i = x0^-1 * w_m^-i from the ctx' inverse-root table.
struct FoldExtArgs {
    FoldArgs base;      // evals/out count ELEMENTS of 4 words; base.coef = Montgomery form of x0^-1
    ExtFactor beta_half;
};
__global__ void __launch_bounds__(256) fri_fold_ext_kernel(const FoldExtArgs fa) {
    const FoldArgs& f = fa.base;
    const uint64_t half = f.half;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint4* ea = reinterpret_cast<const uint4*>(f.evals);
    const uint4* eb = ea + half;
    uint4* o = reinterpret_cast<uint4*>(f.out);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += stride) {
        const uint32_t scaleR = mont_mul(subdomain_mont(f.dom, (uint32_t)i), f.coef);
        const uint4 a = ea[i], b = eb[i];
        const Ext4 r = fold_ext_one(Ext4{{a.x, a.y, a.z, a.w}}, Ext4{{b.x, b.y, b.z, b.w}}, scaleR, fa.beta_half);
        o[i] = make_uint4(r.c[0], r.c[1], r.c[2], r.c[3]);
    }
}

// The same sweep with the folded layer's leaf hashes in it (fold_ext_commit_one, prover_kernels.hpp; include/toyni_hip.h 3j):
// leaves[i] = SHA256(00 || salt_i || out[i].to_bytes()), the row leaf of width 4 that toyni_merkle_commit_rows_device would compute from
// a second read of the layer.  One output and ONE compression per thread, like fri_fold_kernel<.., COMMIT>: hash-bound, so as wide as
// the leaf kernel and never shaped as a stream.
template <bool SALTED>
__global__ void __launch_bounds__(256) fri_fold_ext_commit_kernel(const FoldExtArgs fa, const uint4* __restrict__ salts, Digest* __restrict__ leaves) {
    const FoldArgs& f = fa.base;
    const uint64_t half = f.half;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint4* ea = reinterpret_cast<const uint4*>(f.evals);
    const uint4* eb = ea + half;
    uint4* o = reinterpret_cast<uint4*>(f.out);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += stride) {
        const uint32_t scaleR = mont_mul(subdomain_mont(f.dom, (uint32_t)i), f.coef);
        const uint4 a = ea[i], b = eb[i];
        uint32_t sw[4] = {0u, 0u, 0u, 0u};
        if constexpr (SALTED) {
            const uint4 s = salts[i];
            sw[0] = s.x; sw[1] = s.y; sw[2] = s.z; sw[3] = s.w;
        }
        const FoldExtLeaf r = fold_ext_commit_one<SALTED>(Ext4{{a.x, a.y, a.z, a.w}}, Ext4{{b.x, b.y, b.z, b.w}}, scaleR, fa.beta_half, sw);
        o[i] = make_uint4(r.folded.c[0], r.folded.c[1], r.folded.c[2], r.folded.c[3]);
        leaves[i] = r.leaf;
    }
}

// The same for large layers in the shape of fri_fold_stream_kernel: T-thread workgroups, U load pairs in flight per lane, U * T
// consecutive elements per workgroup and iteration, non-temporal when the layer is far larger than the Infinity Cache.
template <bool NT, int T, int U>
__global__ void __launch_bounds__(T) fri_fold_ext_stream_kernel(const FoldExtArgs fa) {
    const FoldArgs& f = fa.base;
    const uint64_t half = f.half;
    const uint4* ea = reinterpret_cast<const uint4*>(f.evals);
    const uint4* eb = ea + half;
    uint4* o = reinterpret_cast<uint4*>(f.out);
    const uint64_t chunk = (uint64_t)U * T;
    for (uint64_t c0 = (uint64_t)blockIdx.x * chunk; c0 < half; c0 += (uint64_t)gridDim.x * chunk) {
        uint4 a[U], b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = c0 + (uint64_t)u * T + threadIdx.x;
            if (i < half) {
                if constexpr (NT) {
                    const u32x4 va = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ea + i));
                    const u32x4 vb = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(eb + i));
                    a[u] = make_uint4(va.x, va.y, va.z, va.w);
                    b[u] = make_uint4(vb.x, vb.y, vb.z, vb.w);
                } else {
                    a[u] = ea[i];
                    b[u] = eb[i];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t i = c0 + (uint64_t)u * T + threadIdx.x;
            if (i < half) {
                const uint32_t scaleR = mont_mul(subdomain_mont(f.dom, (uint32_t)i), f.coef);
                const Ext4 r = fold_ext_one(Ext4{{a[u].x, a[u].y, a[u].z, a[u].w}}, Ext4{{b[u].x, b[u].y, b[u].z, b[u].w}}, scaleR, fa.beta_half);
                if constexpr (NT) {
                    u32x4 vr = {r.c[0], r.c[1], r.c[2], r.c[3]};
                    __builtin_nontemporal_store(vr, reinterpret_cast<u32x4*>(o + i));
                } else {
                    o[i] = make_uint4(r.c[0], r.c[1], r.c[2], r.c[3]);
                }
            }
        }
    }
}

// explicit base-field points (the reference's signature fri_fold_ext(evals, xs, beta))
__global__ void __launch_bounds__(256) fri_fold_ext_xs_kernel(const uint4* __restrict__ evals, const uint32_t* __restrict__ xs,
                                                               uint4* __restrict__ out, uint64_t half, const ExtFactor beta_half) {
    // a workgroup covers 4 * 256 consecutive elements per iteration and a thread takes element tid of each of the four runs of 256:
    // every wave access is consecutive memory (the four points behind one inversion need not be neighbours)
    const uint64_t chunk = 4u * 256u;
    for (uint64_t c0 = (uint64_t)blockIdx.x * chunk; c0 < half; c0 += (uint64_t)gridDim.x * chunk) {
        uint32_t x[4], xinvR[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t i = c0 + (uint64_t)j * 256u + threadIdx.x;
            x[j] = i < half ? xs[i] : 1u;
        }
        batch_inverse_scaled<4>(x, 1u, xinvR);   // x_j^-1 R; 0 for a zero point (see fri_fold_xs_kernel)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t i = c0 + (uint64_t)j * 256u + threadIdx.x;
            if (i < half) {
                const uint4 a = evals[i], b = evals[i + half];
                const Ext4 r = fold_ext_one(Ext4{{a.x, a.y, a.z, a.w}}, Ext4{{b.x, b.y, b.z, b.w}}, xinvR[j], beta_half);
                out[i] = make_uint4(r.c[0], r.c[1], r.c[2], r.c[3]);
            }
        }
    }
}

// Merkle commitment (merkle_kernels.hpp): one thread per leaf, then one thread per node, level by level
__global__ void __launch_bounds__(256) merkle_leaf_kernel(const uint32_t* __restrict__ values, const uint4* __restrict__ salts,
                                                           Digest* __restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        Digest d;
        if (salts) {
            const uint4 s = salts[i];
            const uint32_t sw[4] = {s.x, s.y, s.z, s.w};
            d = merkle_leaf(values[i], sw);
        } else {
            d = merkle_leaf(values[i], nullptr);
        }
        out[i] = d;
    }
}
// Leaf hashes of the ROWS of an n x width matrix (merkle_row_leaf_at, merkle_kernels.hpp): one thread per row, the launch shape of
// merkle_leaf_kernel.  LAYOUT x SALTED = four instantiations and no more: whether a row-major matrix takes 16-byte loads is a
// uniform run-time flag (`vec`), not a third parameter.  Row-major lanes are `width` words apart: correct for every width, meant
// for narrow rows (an Ext vector is width 4).
static_assert(ROWS_COLUMN_MAJOR == TOYNI_ROWS_COLUMN_MAJOR && ROWS_ROW_MAJOR == TOYNI_ROWS_ROW_MAJOR, "layout codes of the header");
template <int LAYOUT, bool SALTED>
__global__ void __launch_bounds__(256) merkle_rows_leaf_kernel(const uint32_t* __restrict__ values, const uint4* __restrict__ salts,
                                                                Digest* __restrict__ out, size_t n, uint32_t width, size_t col_stride, bool vec) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t sw[4] = {0u, 0u, 0u, 0u};
        if constexpr (SALTED) {
            const uint4 s = salts[i];
            sw[0] = s.x; sw[1] = s.y; sw[2] = s.z; sw[3] = s.w;
        }
        out[i] = merkle_row_leaf_at<LAYOUT, SALTED>(values, i, width, col_stride, vec, sw);
    }
}

// One thread per node: the levels large enough to fill the chip.  (Round 3 also tried block 2's schedule from the SHA_B2 table here --
// 480 instructions fewer per hash, 64 gathers more: 246 against 253 us for the 2^20-leaf FRI round, nothing on a whole proof; not kept.)
__global__ void __launch_bounds__(256) merkle_level_kernel(const Digest* __restrict__ cur, Digest* __restrict__ next, size_t m, size_t up) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < up; i += stride) {
        const Digest l = cur[2 * i];
        const Digest r = (2 * i + 1 < m) ? cur[2 * i + 1] : l;  // odd level: duplicate the last node (src/merkle.rs:38-42)
        next[i] = merkle_node(l, r);
    }
}

// ---- the node hash on two waves (merkle_kernels.hpp, "a node hash on TWO waves") ----
__device__ const ShaB2Table SHA_B2 = make_sha_b2_table();   // K + W of a node's second block for each value of its one data byte (64 KiB)

// One node per lane of a MAIN wave, its HELPER wave (the next wave of the workgroup: another SIMD) computing block 1's message
// schedule.  Both roles, and pairs that have no node at this level (active == false), execute both barriers.  All reads of the
// children happen before the first barrier.  helper / active are wave-uniform (SGPR conditions: scalar branches, not masks).
__device__ inline Digest merkle_node_coop(const Digest& l, const Digest& r, uint32_t* sched, uint32_t lane, bool helper, bool active) {
    uint32_t w[16], last = 0u, kw2[64];
    ShaRegs st{};
    if (active) {
        node_block1(l, r, w, last);
        if (helper) {
            coop_helper_schedule<16, 24>(w, sched, lane);
        } else {
#pragma unroll
            for (int i = 0; i < 64; ++i) kw2[i] = SHA_B2.kw[i][last];   // 64 gathers from a 64 KiB table, in flight while block 1 runs
            coop_main_first16(st, w);
        }
    }
    TOYNI_LDS_BARRIER();
    if (active) {
        if (helper) coop_helper_schedule<40, 24>(w, sched, lane);
        else coop_main_rounds<16>(st, sched, lane);
    }
    TOYNI_LDS_BARRIER();
    Digest d{};
    if (active && !helper) {
        coop_main_rounds<40>(st, sched, lane);
        d = coop_main_finish(st, kw2);
    }
    return d;
}

// A level of up <= 2^15 nodes (the chip cannot be filled: one plain wave per 64 nodes would leave most SIMDs idle anyway): 128-thread
// workgroups, one main + one helper wave per 64 nodes.  Lanes past the end hash the last node again and store nothing.
__global__ void __launch_bounds__(128) merkle_level_coop_kernel(const Digest* __restrict__ cur, Digest* __restrict__ next, size_t m, size_t up) {
    __shared__ uint32_t sched[COOP_SCHED_WORDS];
    const uint32_t lane = threadIdx.x & 63u;
    const bool helper = TOYNI_UNIFORM(threadIdx.x >> 6) != 0;
    const size_t i0 = (size_t)blockIdx.x * 64u + lane;
    const size_t i = i0 < up ? i0 : up - 1;
    const Digest l = cur[2 * i];
    const Digest r = (2 * i + 1 < m) ? cur[2 * i + 1] : l;  // odd level: duplicate the last node (src/merkle.rs:38-42)
    const Digest d = merkle_node_coop(l, r, sched, lane, helper, true);
    if (!helper && i0 < up) next[i0] = d;
}

// All remaining levels of a tree whose current level has m <= MERKLE_TAIL digests, in ONE workgroup: the level lives in
// LDS, each round halves it (odd rounds duplicate the last node) and is also written to global memory (the proofs need
// every level).  Replaces ~log2(m) tiny launches per tree -- the FRI layers of a proof are mostly trees this small.
// Round 3: every level here runs the two-wave node hash: 8 waves = 4 main / helper pairs, up to 256 nodes per level.
constexpr uint32_t MERKLE_TAIL = 512;
constexpr uint32_t MERKLE_TAIL_T = 512;
// `notify` (optional): 9 words of pinned host memory -- the root, then a sequence number stored with system-scope release once
// the root is there.  The host polls that word instead of paying a copy and a stream synchronisation for 32 bytes.
__device__ inline void merkle_notify(const Digest& root, uint32_t* notify, uint32_t seq) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&root);
#pragma unroll
    for (int k = 0; k < 8; ++k) __hip_atomic_store(notify + k, w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(notify + 8, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void merkle_notify_kernel(const Digest* __restrict__ root, uint32_t* notify, uint32_t seq) {
    if (threadIdx.x == 0 && blockIdx.x == 0) merkle_notify(*root, notify, seq);
}
__global__ void __launch_bounds__(MERKLE_TAIL_T) merkle_tail_kernel(const Digest* __restrict__ cur, Digest* __restrict__ next, uint32_t m,
                                                                    uint32_t* notify, uint32_t seq) {
    __shared__ Digest lvl[MERKLE_TAIL];
    __shared__ uint32_t sched[MERKLE_TAIL_T / 128][COOP_SCHED_WORDS];
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) lvl[i] = cur[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = TOYNI_UNIFORM(threadIdx.x >> 6);
    const uint32_t pair = wave >> 1;
    const bool helper = (wave & 1u) != 0u;
    while (m > 1) {
        const uint32_t up = (m + 1) / 2;
        const bool active = pair * 64u < up;               // wave-uniform
        const uint32_t i0 = pair * 64u + lane;
        const uint32_t i = i0 < up ? i0 : up - 1;
        Digest l{}, r{};
        if (active) {
            l = lvl[2 * i];
            r = (2 * i + 1 < m) ? lvl[2 * i + 1] : l;
        }
        const Digest d = merkle_node_coop(l, r, sched[pair], lane, helper, active);   // its first barrier: every read of the old level is done
        if (active && !helper && i0 < up) {
            lvl[i0] = d;
            next[i0] = d;
        }
        TOYNI_LDS_BARRIER();
        next += up;
        m = up;
    }
    if (notify && threadIdx.x == 0) merkle_notify(lvl[0], notify, seq);
}

// ---- the Fiat-Shamir transcript in device memory (transcript_kernels.hpp; include/toyni_hip.h 3l) ----
// Every kernel here is ONE wave: the chains are serial, one lane runs them; the lanes share only the byte copy of an absorb and, in
// the index squeeze (where every lane computes the same hashes: uniform branches throughout), the search of the values seen so far.
static_assert(sizeof(toyni_transcript) == sizeof(TranscriptState) && offsetof(toyni_transcript, bytes) == offsetof(TranscriptState, bytes) &&
              offsetof(toyni_transcript, status) == offsetof(TranscriptState, status) && TOYNI_TRANSCRIPT_CAPACITY == TRANSCRIPT_CAPACITY &&
              TOYNI_E_RANGE == TRANSCRIPT_E_RANGE, "toyni_transcript of the header");
constexpr uint32_t TRANSCRIPT_T = 64;
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_absorb_kernel(TranscriptState* __restrict__ tr, const uint8_t* __restrict__ src, uint32_t n) {
    transcript_absorb_wave(*tr, src, n, threadIdx.x, TRANSCRIPT_T);
}
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_squeeze_kernel(TranscriptState* __restrict__ tr, uint32_t* __restrict__ out, uint32_t count) {
    if (threadIdx.x == 0) transcript_squeeze(*tr, out, count);
}
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_squeeze_indices_kernel(TranscriptState* __restrict__ tr, uint32_t count, uint32_t max,
                                                                                   uint32_t* __restrict__ out) {
    __shared__ uint32_t seen[TRANSCRIPT_MAX_INDICES];
    __shared__ uint32_t flag;
    // "some lane found it": through one LDS word.  The LDS operations of a wave execute in program order, so clear / set / read need
    // no barrier, only the compiler kept from moving them.
    const auto any_lane = [](bool hit) {
        if (threadIdx.x == 0) flag = 0u;
        TOYNI_WAVE_ORDER();
        if (hit) flag = 1u;
        TOYNI_WAVE_ORDER();
        const uint32_t some = flag;
        TOYNI_WAVE_ORDER();
        return some != 0u;
    };
    transcript_squeeze_indices(*tr, count, max, out, seen, threadIdx.x, TRANSCRIPT_T, any_lane);
}
__global__ void __launch_bounds__(256) fri_query_positions_kernel(const uint32_t* __restrict__ indices, uint32_t count, uint64_t m0, uint64_t total,
                                                                  uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) out[t] = fri_query_position(indices, count, m0, t);
}

// ---- from the quotient root onward without the host (dz_kernels.hpp; include/toyni_hip.h 3o) ----
// The preparation kernels are ONE wave each: what they compute is a handful of dependent Ext products per point (or per term), far
// below what a launch costs, and a wave needs no barrier.  The hot kernels are the bodies of 3h with the z-dependent constants read
// from the record those kernels leave in the stream's buffer instead of from the kernel arguments.
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_squeeze_ext_point_kernel(TranscriptState* __restrict__ tr, uint32_t* __restrict__ z) {
    if (threadIdx.x == 0) transcript_squeeze_ext_point(*tr, z);
}
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_absorb_fields_kernel(TranscriptState* __restrict__ tr, const uint32_t* __restrict__ words,
                                                                                 uint32_t count) {
    transcript_absorb_fields_wave(*tr, words, count, threadIdx.x, TRANSCRIPT_T);
}
__global__ void __launch_bounds__(256) query_rows_kernel(const uint32_t* __restrict__ indices, const QueryRowOffsets off, uint32_t noffsets, uint64_t n,
                                                         uint64_t total, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) out[t] = query_row(indices, off, noffsets, n, t);
}
// lane p: the two tables of point mults[p] * z
__global__ void __launch_bounds__(TRANSCRIPT_T) poly_ext_prepare_kernel(const uint32_t* __restrict__ z, const PolyDzMults mults, uint32_t npoints,
                                                                        PolyExtRecord* __restrict__ rec) {
    if (threadIdx.x < npoints) poly_ext_record_point(z, mults.v[threadIdx.x], rec->thread[threadIdx.x], rec->chunk[threadIdx.x]);
}
__global__ void __launch_bounds__(256) poly_eval_ext_batch_partial_dz_kernel(const PolyExtDzArgs a, const PolyExtRecord* __restrict__ rec) {
    __shared__ uint32_t red[256];
    for (uint32_t col = blockIdx.y; col < a.batch; col += gridDim.y) {
        uint32_t c[POLY_PER_THREAD];
        poly_ext_load(a, col, blockIdx.x, threadIdx.x, c);
        for (uint32_t p = 0; p < a.npoints; ++p) {
            const Ext4 v = poly_ext_thread_term(rec->thread[p], c, threadIdx.x);
            uint32_t* dst = a.partial + poly_ext_partial_index(a, col, blockIdx.x, p);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t sum = block_sum_mod(v.c[k], red);
                if (threadIdx.x == 0) dst[k] = sum;
            }
        }
    }
}
__global__ void __launch_bounds__(256) poly_eval_ext_batch_final_dz_kernel(const PolyExtDzArgs a, const PolyExtRecord* __restrict__ rec) {
    __shared__ uint32_t red[256];
    for (uint32_t col = blockIdx.x; col < a.batch; col += gridDim.x)
        for (uint32_t p = 0; p < a.npoints; ++p) {
            const Ext4 v = poly_ext_final_thread(a, rec->chunk[p], col, p, threadIdx.x);
            uint32_t* dst = a.out + ((uint64_t)col * a.npoints + p) * 4u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t sum = block_sum_mod(v.c[k], red);
                if (threadIdx.x == 0) dst[k] = sum;
            }
        }
}
// the slots inside the kernel arguments (capturable) ...
__global__ void __launch_bounds__(TRANSCRIPT_T) deep_ext_prepare_inline_kernel(const DeepExtInlineSlots in, uint32_t nslots, const uint32_t* __restrict__ z,
                                                                               const uint32_t* __restrict__ alphas, const uint32_t* __restrict__ claims,
                                                                               DeepExtRecord* __restrict__ rec) {
    __shared__ uint32_t part[4 * TRANSCRIPT_T];
    deep_ext_prepare(in.s, nslots, z, alphas, claims, rec, part, threadIdx.x, TRANSCRIPT_T);
}
// ... or in device memory (any length)
__global__ void __launch_bounds__(TRANSCRIPT_T) deep_ext_prepare_kernel(const DeepExtSlot* __restrict__ slots, uint32_t nslots, const uint32_t* __restrict__ z,
                                                                        const uint32_t* __restrict__ alphas, const uint32_t* __restrict__ claims,
                                                                        DeepExtRecord* __restrict__ rec) {
    __shared__ uint32_t part[4 * TRANSCRIPT_T];
    deep_ext_prepare(slots, nslots, z, alphas, claims, rec, part, threadIdx.x, TRANSCRIPT_T);
}
// deep_combine_ext_kernel with C, adj_z, m_z and the table from the record
__global__ void __launch_bounds__(256) deep_combine_ext_dz_kernel(const DeepExtArgs a, const DeepExtRecord* __restrict__ rec) {
    DeepExtArgs b = a;
    deep_ext_args_from_record(b, *rec);
    deep_combine_ext_body(b, deep_ext_record_table(rec));
}

// ---- gamma and the constraint weights without the host (dc_kernels.hpp; include/toyni_hip.h 3p) ----
// Two more one-wave preparation kernels, and the hot kernels of 3i and 3k with what depends on a challenge read from the record the
// preparation left in the stream's buffer.  The argument-fed kernels above are not touched: each twin is a kernel of its own.
__global__ void __launch_bounds__(TRANSCRIPT_T) air_dc_prepare_kernel(const uint32_t* __restrict__ params, uint32_t nparams,
                                                                      const uint32_t* __restrict__ alphas, uint32_t nalphas, uint32_t form,
                                                                      uint32_t* __restrict__ rec) {
    air_dc_prepare(params, nparams, alphas, nalphas, form, rec, threadIdx.x, TRANSCRIPT_T);
}
// air_quotient_ext_kernel with the parameters and the weights from the record: rec[0 .. nparams) Montgomery forms, then the weights
__global__ void __launch_bounds__(256) air_quotient_ext_dc_kernel(const AirArgs a, const uint64_t out_stride, const uint32_t* __restrict__ rec,
                                                                  const uint32_t nparams) {
    constexpr int K = 4;
    const uint32_t* weights4 = rec + nparams;
    const uint32_t B = 1u << a.log_blowup;
    uint32_t* zh_lds = air_lds + a.nregs * blockDim.x * K;
    if (a.zh_lds) {
        for (uint32_t t = threadIdx.x; t < B; t += blockDim.x) zh_lds[t] = zh_inv_class(a.shift_nR, a.wBR, t);
        __syncthreads();
    }
    const uint64_t N = (uint64_t)1 << a.log_N;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.log_N >= 2) {
        if (g >= N / K) return;
        const uint64_t i0 = g * K;
        uint32_t zhR[K], c[4][K], q[4][K];
        if (a.zh_lds) {
#pragma unroll
            for (int j = 0; j < K; ++j) zhR[j] = zh_lds[(i0 + j) & (B - 1)];
        } else if (a.divides) {
            air_zh_inverses<K>(a, i0, zhR);
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) zhR[j] = 0u;
        }
        air_eval_group_ext_dc<K>(a, rec, weights4, air_lds + threadIdx.x * K, blockDim.x * K, i0, zhR, c, q);
        air_ext_store<K>(a.c_out, out_stride, i0, a.accumulate, c);
        air_ext_store<K>(a.q_out, out_stride, i0, a.accumulate, q);
    } else if (g < N) {
        uint32_t zhR[1] = {0u}, c[4][1], q[4][1];
        if (a.zh_lds) zhR[0] = zh_lds[g & (B - 1)];
        else if (a.divides) air_zh_inverses<1>(a, g, zhR);
        air_eval_group_ext_dc<1>(a, rec, weights4, air_lds + threadIdx.x, blockDim.x, g, zhR, c, q);
        air_ext_store<1>(a.c_out, out_stride, g, a.accumulate, c);
        air_ext_store<1>(a.q_out, out_stride, g, a.accumulate, q);
    }
}
__global__ void __launch_bounds__(TRANSCRIPT_T) extcol_dc_prepare_kernel(const uint32_t* __restrict__ challenges, uint32_t num_index, uint32_t den_index,
                                                                            uint32_t den_norm, ExtAccumRecord* __restrict__ rec) {
    ext_accum_dc_prepare(challenges, num_index, den_index, den_norm, rec, threadIdx.x);
}
// steps 1 and 3 of 3i with the shifts and adj_z / m_z from the record (step 2 reads no operand and is launched as it is)
template <int OP>
__global__ void __launch_bounds__(EXT_ACCUM_THREADS) extcol_aggregate_dc_kernel(const ExtAccumArgs a, const ExtAccumRecord* __restrict__ rec) {
    __shared__ Ext4 wave_tot[EXT_ACCUM_THREADS / SCAN_WAVE];
    __shared__ uint32_t wave_zeros[EXT_ACCUM_THREADS / SCAN_WAVE];
    ExtAccumArgs b = a;
    ext_accum_args_from_record(b, *rec);
    ext_accum_aggregate_body<OP>(b, wave_tot, wave_zeros);
}
template <int OP>
__global__ void __launch_bounds__(EXT_ACCUM_THREADS) extcol_apply_dc_kernel(const ExtAccumArgs a, const ExtAccumSeeds in,
                                                                               const ExtAccumRecord* __restrict__ rec) {
    __shared__ Ext4 wave_tot[EXT_ACCUM_THREADS / SCAN_WAVE];
    __shared__ uint32_t wave_zeros[EXT_ACCUM_THREADS / SCAN_WAVE];
    ExtAccumArgs b = a;
    ext_accum_args_from_record(b, *rec);
    ext_accum_apply_body<OP>(b, in, wave_tot, wave_zeros);
}

// ---- the base-field first half of a Fibonacci proof without the host (fib_dz_kernels.hpp; include/toyni_hip.h 3q) ----
// One-wave preparation kernels again, and twins of the three hot kernels of 3c that read z (and the claimed values) from the record
// the preparation left in the stream's buffer.  The argument-fed kernels above are not touched.
__global__ void __launch_bounds__(256) fib_mask_kernel(const FibMaskArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= fib_mask_items(a.n, a.mask_degree)) return;
    const uint64_t j = fib_mask_item_word(a.n, a.mask_degree, t);
    a.coeffs[j] = fib_mask_output(a, j, a.coeffs[j]);
}
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_squeeze_point_kernel(TranscriptState* __restrict__ tr, uint32_t log_N, uint32_t shift_invR,
                                                                                 uint32_t* __restrict__ z) {
    if (threadIdx.x == 0) transcript_squeeze_point(*tr, log_N, shift_invR, FIB_POINT_TRIES, z);
}
// lane p: the three powers of point mults[p] * z
__global__ void __launch_bounds__(TRANSCRIPT_T) poly_dz_prepare_kernel(const uint32_t* __restrict__ z, const PolyDzMults mults, uint32_t npoints,
                                                                       PolyDzRecord* __restrict__ rec) {
    if (threadIdx.x < npoints) poly_dz_record_point(z, mults.v[threadIdx.x], threadIdx.x, *rec);
}
__global__ void __launch_bounds__(256) poly_eval_partial_dz_kernel(const PolyEvalDzArgs a, const PolyDzRecord* __restrict__ rec) {
    __shared__ uint32_t red[256];
    const uint64_t base = (uint64_t)blockIdx.x * POLY_CHUNK + (uint64_t)threadIdx.x * POLY_PER_THREAD;
    uint32_t c[POLY_PER_THREAD];
#pragma unroll
    for (uint32_t j = 0; j < POLY_PER_THREAD; ++j) c[j] = base + j < a.ncoeffs ? a.coeffs[base + j] : 0u;
    for (uint32_t p = 0; p < a.npoints; ++p) {
        const uint32_t sum = block_sum_mod(poly_thread_term(poly_dz_point_args(rec, p), 0u, c, threadIdx.x), red);
        if (threadIdx.x == 0) a.partial[(uint64_t)blockIdx.x * a.npoints + p] = sum;
    }
}
__global__ void __launch_bounds__(256) poly_eval_final_dz_kernel(const PolyEvalDzArgs a, const PolyDzRecord* __restrict__ rec) {
    __shared__ uint32_t red[256];
    for (uint32_t p = 0; p < a.npoints; ++p) {
        const uint32_t zchunkR = TOYNI_UNIFORM_LOAD(&rec->zchunkR[p]);
        uint32_t acc = 0;
        for (uint32_t b = threadIdx.x; b < a.nblocks; b += blockDim.x)
            acc = bb_add(acc, mont_mul(a.partial[(uint64_t)b * a.npoints + p], mont_pow(zchunkR, b)));
        const uint32_t sum = block_sum_mod(acc, red);
        if (threadIdx.x == 0) a.out[p] = sum;
    }
}
__global__ void __launch_bounds__(TRANSCRIPT_T) fib_deep_prepare_kernel(const uint32_t* __restrict__ z, const uint32_t* __restrict__ ood, const FibCheckArgs k,
                                                                        FibDeepRecord* __restrict__ rec, uint32_t* __restrict__ check) {
    if (threadIdx.x == 0) fib_deep_prepare(z, ood, k, rec, check);
}
// fib_deep_kernel with z and the claimed values from the record
__global__ void __launch_bounds__(256) fib_deep_dz_kernel(const DeepArgs in, const FibDeepRecord* __restrict__ rec) {
    constexpr int K = 8;
    DeepArgs a = in;
    fib_deep_args_from_record(a, *rec);
    const uint64_t N = (uint64_t)1 << a.log_N, mask = N - 1, B = (uint64_t)1 << a.log_blowup;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    if (a.log_N >= 3) {
        for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < N / K; g += stride) {
            const uint64_t i0 = g * K;
            uint32_t t0[K], t1[K], t2[K], qv[K], out[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                t0[j] = a.trace[i0 + j];
                t1[j] = a.trace[(i0 + j + B) & mask];
                t2[j] = a.trace[(i0 + j + 2 * B) & mask];
                qv[j] = a.quot[i0 + j];
            }
            deep_group<K>(a, i0, t0, t1, t2, qv, out);
#pragma unroll
            for (int j = 0; j < K; ++j) a.out[i0 + j] = out[j];
        }
    } else {
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
            const uint32_t t0[1] = {a.trace[i]}, t1[1] = {a.trace[(i + B) & mask]}, t2[1] = {a.trace[(i + 2 * B) & mask]}, qv[1] = {a.quot[i]};
            uint32_t out[1];
            deep_group<1>(a, i, t0, t1, t2, qv, out);
            a.out[i] = out[0];
        }
    }
}
__global__ void __launch_bounds__(256) fri_phase_roots_kernel(const uint32_t* __restrict__ levels, uint64_t m_first, uint32_t rounds, uint32_t* __restrict__ roots) {
    for (uint32_t t = threadIdx.x; t < 8u * rounds; t += blockDim.x) roots[t] = fri_phase_root_word(levels, m_first, t);
}

// ---- a proof-of-work nonce on that transcript (pow_kernels.hpp; include/toyni_hip.h 3n) ----
// One chain of three launches on one word of device memory: arm (one wave), search (the whole chip), finish (one wave).  The search
// waits for nothing: a workgroup hashes the state's full blocks once on one lane (the midstate, through LDS behind the kernel's only
// barrier), then every thread walks its candidates until pow_stop says that none of them can be the minimum any more.
__global__ void __launch_bounds__(TRANSCRIPT_T) pow_arm_kernel(TranscriptState* __restrict__ tr, uint64_t* __restrict__ nonce) {
    if (threadIdx.x == 0) pow_arm(*tr, nonce);
}
// The state's length lives in device memory, so the host cannot choose between the one-block and the two-block candidate: ONE kernel
// holds both instantiations of the loop and takes one of them on a value that is the same in every thread of the launch -- a branch
// around the loops, none inside them.
template <bool TWO>
__device__ __forceinline__ void pow_search_body(const TranscriptState& tr, uint32_t len, const Sha256State& mid, uint32_t bits, uint64_t start,
                                                uint64_t tries, uint64_t* best) {
    const PowTail<TWO> tail = pow_tail<TWO>(tr, len);
    pow_search<TWO>(mid, tail, len & 63u, bits, start, tries, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, (uint64_t)gridDim.x * blockDim.x, best);
}
__global__ void __launch_bounds__(POW_T) pow_search_kernel(const TranscriptState* __restrict__ tr, uint32_t bits, uint64_t start, uint64_t tries,
                                                           uint64_t* best) {
    __shared__ Sha256State mid;
    if (tr->status != 0u) return;                                   // the same in every thread: nobody is left at the barrier
    const uint32_t len = TOYNI_UNIFORM(tr->len);
    if (threadIdx.x == 0) mid = pow_midstate(*tr, len);
    __syncthreads();
    const Sha256State m = mid;
    if (pow_two_blocks(len)) pow_search_body<true>(*tr, len, m, bits, start, tries, best);
    else pow_search_body<false>(*tr, len, m, bits, start, tries, best);
}
__global__ void __launch_bounds__(TRANSCRIPT_T) pow_finish_kernel(TranscriptState* __restrict__ tr, uint64_t* __restrict__ nonce, uint32_t bits,
                                                                  uint32_t top) {
    if (threadIdx.x == 0) pow_finish(*tr, nonce, bits, top != 0u);
}

// ---- the commit phase on that transcript (include/toyni_hip.h 3l) ----
// Between two rounds, one wave: absorb the root the tree's last kernel has just written (root != nullptr), then squeeze the next
// round's beta (nsqueeze = 1, or 4 for an Ext beta; 0 after the last round) and leave it in device memory in the form the next fold
// consumes -- the host cannot: it never sees beta.  rec[k] = beta_k c0 in Montgomery form, rec[4 + k] = beta_k c1 likewise (Ext
// only), c0 / c1 = host constants times R^2: base c0 = 1 / (2 x_k); Ext c0 = 1 / 2, c1 = 11 / 2, which makes rec an ExtFactor of
// beta / 2.  betas (optional) receives the plain canonical coordinates.  A transcript whose status is set gives beta = 0.
__global__ void __launch_bounds__(TRANSCRIPT_T) fri_transcript_round_kernel(TranscriptState* __restrict__ tr, const uint8_t* __restrict__ root,
                                                                             uint32_t nsqueeze, uint32_t c0, uint32_t c1, uint32_t* __restrict__ rec,
                                                                             uint32_t* __restrict__ betas) {
    __shared__ uint32_t beta[4];
    if (threadIdx.x == 0) {
        if (root) transcript_absorb(*tr, root, 32u);
        transcript_squeeze(*tr, beta, nsqueeze);
    }
    if (nsqueeze == 0u) return;
    __syncthreads();
    if (threadIdx.x < nsqueeze) {
        const uint32_t b = beta[threadIdx.x];
        if (betas) betas[threadIdx.x] = b;
        rec[threadIdx.x] = transcript_factor(b, c0);
        if (nsqueeze == 4u) rec[4u + threadIdx.x] = transcript_factor(b, c1);
    }
}

// The folds of that phase: fri_fold_kernel<.., COMMIT> and fri_fold_ext_commit_kernel with the challenge's factor read from the
// record the kernel above left, instead of from the launch arguments.  One output and one leaf hash per thread, grid-stride.
__global__ void __launch_bounds__(256) fri_fold_commit_rec_kernel(const FoldArgs f0, const uint32_t* __restrict__ rec, const uint4* __restrict__ salts,
                                                                  Digest* __restrict__ leaves) {
    FoldArgs f = f0;
    f.coef = rec[0];
    const uint64_t half = f.half;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += stride) {
        const uint32_t r = fold_one(f, i, f.evals[i], f.evals[i + half]);
        f.out[i] = r;
        if (salts) {
            const uint4 sv = salts[i];
            const uint32_t sw[4] = {sv.x, sv.y, sv.z, sv.w};
            leaves[i] = merkle_leaf(r, sw);
        } else {
            leaves[i] = merkle_leaf(r, nullptr);
        }
    }
}
template <bool SALTED>
__global__ void __launch_bounds__(256) fri_fold_ext_commit_rec_kernel(const FoldArgs f, const ExtFactor* __restrict__ rec, const uint4* __restrict__ salts,
                                                                      Digest* __restrict__ leaves) {
    const ExtFactor beta_half = *rec;
    const uint64_t half = f.half;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint4* ea = reinterpret_cast<const uint4*>(f.evals);
    const uint4* eb = ea + half;
    uint4* o = reinterpret_cast<uint4*>(f.out);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += stride) {
        const uint32_t scaleR = mont_mul(subdomain_mont(f.dom, (uint32_t)i), f.coef);
        const uint4 a = ea[i], b = eb[i];
        uint32_t sw[4] = {0u, 0u, 0u, 0u};
        if constexpr (SALTED) {
            const uint4 s = salts[i];
            sw[0] = s.x; sw[1] = s.y; sw[2] = s.z; sw[3] = s.w;
        }
        const FoldExtLeaf r = fold_ext_commit_one<SALTED>(Ext4{{a.x, a.y, a.z, a.w}}, Ext4{{b.x, b.y, b.z, b.w}}, scaleR, beta_half, sw);
        o[i] = make_uint4(r.folded.c[0], r.folded.c[1], r.folded.c[2], r.folded.c[3]);
        leaves[i] = r.leaf;
    }
}

// ---- four-to-one Ext FRI rounds under coset leaves (include/toyni_hip.h 3m) ----
// One thread per LEAF of the folded layer (fold4_ext_commit_leaf, prover_kernels.hpp): the 16 input elements t + k m/16, k < 16 --
// sixteen 16-byte loads, each one consecutive across the lanes of a wave --, 12 pairwise folds, the four outputs t + q m/16 and the
// three compressions of the leaf from the folded words in registers.  No LDS, no barrier.  Hash-bound (three compressions against
// about a third of one in folding), so the wide grid-stride shape of fri_fold_ext_commit_kernel and never a stream shape.  The four
// outputs of a leaf are m / 16 apart: a mapping with one output per lane could not hash the leaf without an exchange.
struct Fold4ExtArgs {
    const uint32_t* evals;   // m Ext elements
    uint32_t* out;           // m / 4 Ext elements
    SubDomain dom;           // winv_N^(i << s) for i < m (Montgomery)
    uint32_t xinvR;          // Montgomery form of x0^-1
    uint32_t iinvR;          // Montgomery form of w_4^-1
    uint64_t leaves;         // m / 16
};
template <bool SALTED>
__device__ __forceinline__ void fold4_ext_commit_sweep(const Fold4ExtArgs& a, const ExtFactor& f1, const ExtFactor& f2, const uint4* __restrict__ salts,
                                                       Digest* __restrict__ leaves) {
    const uint64_t nl = a.leaves;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint4* e = reinterpret_cast<const uint4*>(a.evals);
    uint4* o = reinterpret_cast<uint4*>(a.out);
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nl; t += stride) {
        Ext4 in[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint4 v = e[t + (uint64_t)k * nl];
            in[k] = Ext4{{v.x, v.y, v.z, v.w}};
        }
        uint32_t sR[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) sR[q] = mont_mul(subdomain_mont(a.dom, (uint32_t)(t + (uint64_t)q * nl)), a.xinvR);
        uint32_t sw[4] = {0u, 0u, 0u, 0u};
        if constexpr (SALTED) {
            const uint4 s = salts[t];
            sw[0] = s.x; sw[1] = s.y; sw[2] = s.z; sw[3] = s.w;
        }
        const Fold4ExtLeaf r = fold4_ext_commit_leaf<SALTED>(in, sR, a.iinvR, f1, f2, sw);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[t + (uint64_t)q * nl] = make_uint4(r.folded[q].c[0], r.folded[q].c[1], r.folded[q].c[2], r.folded[q].c[3]);
        leaves[t] = r.leaf;
    }
}
struct Fold4ExtFactors { ExtFactor beta_half, beta2_half; };
template <bool SALTED>
__global__ void __launch_bounds__(256) fri_fold4_ext_commit_kernel(const Fold4ExtArgs a, const Fold4ExtFactors f, const uint4* __restrict__ salts,
                                                                   Digest* __restrict__ leaves) {
    fold4_ext_commit_sweep<SALTED>(a, f.beta_half, f.beta2_half, salts, leaves);
}
// its twin for the phase on a device transcript: the two factors from the record fri4_transcript_round_kernel left
template <bool SALTED>
__global__ void __launch_bounds__(256) fri_fold4_ext_commit_rec_kernel(const Fold4ExtArgs a, const Fold4ExtFactors* __restrict__ rec,
                                                                       const uint4* __restrict__ salts, Digest* __restrict__ leaves) {
    const Fold4ExtFactors f = *rec;
    fold4_ext_commit_sweep<SALTED>(a, f.beta_half, f.beta2_half, salts, leaves);
}

// Between two rounds of that phase, one wave: fri_transcript_round_kernel with an Ext beta and a record of TWO factors
// (fri4_round_record: beta / 2 and beta^2 / 2).  The five dependent compressions and the one Ext product run on lane 0.
__global__ void __launch_bounds__(TRANSCRIPT_T) fri4_transcript_round_kernel(TranscriptState* __restrict__ tr, const uint8_t* __restrict__ root,
                                                                              uint32_t squeeze, uint32_t half_r2, uint32_t half11_r2, uint32_t eleven_r2,
                                                                              uint32_t* __restrict__ rec, uint32_t* __restrict__ betas) {
    if (threadIdx.x != 0) return;
    if (root) transcript_absorb(*tr, root, 32u);
    if (squeeze == 0u) return;
    uint32_t beta[4];
    transcript_squeeze(*tr, beta, 4u);
    ExtFactor f[2];
    fri4_round_record(beta, half_r2, half11_r2, eleven_r2, f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (betas) betas[k] = beta[k];
        rec[k] = f[0].b[k]; rec[4 + k] = f[0].b11[k];
        rec[8 + k] = f[1].b[k]; rec[12 + k] = f[1].b11[k];
    }
}

// Coset leaves of a layer as it lies: merkle_row_leaf_at with the internal layout ROWS_EXT_QUARTERS (merkle_kernels.hpp), width 16,
// one thread per leaf in the launch shape of merkle_rows_leaf_kernel.  n = m / 4 leaves.
template <bool SALTED>
__global__ void __launch_bounds__(256) merkle_coset_leaf_kernel(const uint32_t* __restrict__ layer, const uint4* __restrict__ salts,
                                                                Digest* __restrict__ out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t sw[4] = {0u, 0u, 0u, 0u};
        if constexpr (SALTED) {
            const uint4 s = salts[i];
            sw[0] = s.x; sw[1] = s.y; sw[2] = s.z; sw[3] = s.w;
        }
        out[i] = merkle_row_leaf_at<ROWS_EXT_QUARTERS, SALTED>(layer, i, 16u, n, true, sw);
    }
}

// list k < rounds of `count` words: the leaf query q opens in layer k, d_indices[q] mod (m0 >> (2 k + 2))
__global__ void __launch_bounds__(256) fri4_query_positions_kernel(const uint32_t* __restrict__ indices, uint32_t count, uint64_t m0, uint64_t total,
                                                                   uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint64_t k = t / count, leaves = m0 >> (2u * k + 2u);
        out[t] = (uint32_t)(indices[t % count] & (leaves - 1u));
    }
}

// Openings of coset leaves: merkle_open_rows_kernel's record with width 16, the 16 value words of leaf `index` gathered from the four
// quarters of the layer (word c of the leaf = word c mod 4 of element index + (c / 4) n, n = m / 4 leaves).
__global__ void __launch_bounds__(256) merkle_open_cosets_kernel(const OpenRows g) {
    const uint32_t depth = merkle_depth(g.n);
    const uint64_t values_at = (uint64_t)depth * 32u + 16u, flags_at = values_at + 8u * 16u;
    const uint64_t rec = flags_at + ((depth + 7u) & ~7u);
    const uint64_t per = (uint64_t)depth + 1u + 16u, total = (uint64_t)g.nidx * per;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += stride) {
        const uint32_t k = (uint32_t)(w / per);
        const uint64_t item = w % per;
        const uint64_t index = g.indices[k];
        uint8_t* r = g.out + (uint64_t)k * rec;
        if (item < depth) {
            bool is_left;
            const uint64_t row = merkle_sibling_row(g.n, index, (uint32_t)item, is_left);
            reinterpret_cast<Digest*>(r)[item] = g.levels[row];
            r[flags_at + item] = is_left ? 1 : 0;
        } else if (item == depth) {
            uint32_t* tail = reinterpret_cast<uint32_t*>(r + (uint64_t)depth * 32u);
            uint4 sv = make_uint4(0u, 0u, 0u, 0u);
            if (g.salts) sv = g.salts[index];
            tail[0] = sv.x; tail[1] = sv.y; tail[2] = sv.z; tail[3] = sv.w;
            for (uint64_t b = flags_at + depth; b < rec; ++b) r[b] = 0;   // byte stores, clear of the position bytes
        } else {
            const uint64_t c = item - depth - 1u;
            uint32_t* val = reinterpret_cast<uint32_t*>(r + values_at + 8u * c);
            val[0] = coset_value_word(g.values, g.n, index, (uint32_t)c);
            val[1] = 0u;
        }
    }
}

// ALL remaining rounds of a transcript commit phase in ONE workgroup, from the first round whose folded layer has at most MERKLE_TAIL
// leaves: a round that small is a chain of dependent compressions in which every launch boundary costs about what the hash it
// separates does, and with beta produced on the device nothing between two rounds needs the host.  The layer (folded in place: thread
// i reads elements i and i + half and writes element i, which no other thread touches in that round), the tree level, the two-wave
// schedule areas and the transcript itself live in LDS; every layer and every level is also written to global memory.  Per round:
//   thread 0: absorb the previous root (from the level array), squeeze beta                                | barrier
//   thread i < half: fold, leaf hash from the registers that hold the folded element (the last layer unsalted)  | barrier
//   the node levels with merkle_node_coop, as merkle_tail_kernel runs them (its barriers)
// and after the last round thread 0 absorbs the last root and the transcript goes back to global memory.  Round r of the launch folds on
// the points of a.dom at stride 2^r (w_{m/2} = w_m^2) and on x^(2^r): one SubDomain and one x^-1 serve every round.  Every loop count
// and every barrier condition is decided from m: wave-uniform.
struct FriTailArgs {
    const uint32_t* cur;     // the layer the first fused round folds: m elements
    uint32_t* out;           // the folded layers, back to back
    Digest* levels;          // their trees, back to back
    const uint4* salts;      // 16 bytes per leaf of every salted layer back to back (the final layer has none), or nullptr
    TranscriptState* tr;
    uint32_t* betas;         // the plain canonical beta of every round, or nullptr
    SubDomain dom;           // winv_N^(i << s) for the first fused round's m (Montgomery)
    uint32_t m, final_size;
    uint32_t xinvR;          // Montgomery form of 1 / x of the first fused round
    uint32_t half_r2, half11_r2;   // (1 / 2) R^2 and (11 / 2) R^2: transcript_factor
};
template <bool EXT>
__global__ void __launch_bounds__(MERKLE_TAIL_T) fri_tail_rounds_kernel(const FriTailArgs a) {
    constexpr uint32_t W = EXT ? 4u : 1u, NSQ = EXT ? 4u : 1u;
    __shared__ uint32_t layer[2 * MERKLE_TAIL * W];
    __shared__ Digest lvl[MERKLE_TAIL];
    __shared__ uint32_t sched[MERKLE_TAIL_T / 128][COOP_SCHED_WORDS];
    __shared__ TranscriptState tr;
    __shared__ uint32_t beta[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = TOYNI_UNIFORM(tid >> 6);
    const uint32_t pair = wave >> 1;
    const bool helper = (wave & 1u) != 0u;
    for (uint32_t i = tid; i < a.m * W; i += blockDim.x) layer[i] = a.cur[i];
    for (uint32_t i = tid; i < TRANSCRIPT_CAPACITY; i += blockDim.x) tr.bytes[i] = a.tr->bytes[i];
    if (tid == 0) { tr.len = a.tr->len; tr.status = a.tr->status; }
    __syncthreads();
    uint32_t m = a.m, shift = 0, xinvR = a.xinvR;
    uint32_t* out = a.out;
    Digest* levels = a.levels;
    const uint4* salts = a.salts;
    uint32_t* betas = a.betas;
    bool have_root = false;
    while (m > a.final_size) {
        const uint32_t half = m >> 1;
        const bool salted = salts && half != a.final_size;
        if (tid == 0u) {
            if (have_root) transcript_absorb(tr, reinterpret_cast<const uint8_t*>(&lvl[0]), 32u);
            transcript_squeeze(tr, beta, NSQ);
            if (betas) {
#pragma unroll
                for (uint32_t k = 0; k < NSQ; ++k) betas[k] = beta[k];
            }
        }
        __syncthreads();   // beta is there; the root has been read before a leaf of this round replaces it
        if (tid < half) {
            uint32_t sw[4] = {0u, 0u, 0u, 0u};
            if (salted) {
                const uint4 sv = salts[tid];
                sw[0] = sv.x; sw[1] = sv.y; sw[2] = sv.z; sw[3] = sv.w;
            }
            Digest d;
            if constexpr (EXT) {
                ExtFactor f;
#pragma unroll
                for (int k = 0; k < 4; ++k) { f.b[k] = transcript_factor(beta[k], a.half_r2); f.b11[k] = transcript_factor(beta[k], a.half11_r2); }
                const uint32_t scaleR = mont_mul(subdomain_mont(a.dom, tid << shift), xinvR);
                const uint32_t* pa = layer + 4u * tid;
                const uint32_t* pb = layer + 4u * (tid + half);
                const Ext4 va{{pa[0], pa[1], pa[2], pa[3]}}, vb{{pb[0], pb[1], pb[2], pb[3]}};
                const FoldExtLeaf r = salted ? fold_ext_commit_one<true>(va, vb, scaleR, f, sw) : fold_ext_commit_one<false>(va, vb, scaleR, f, sw);
#pragma unroll
                for (int k = 0; k < 4; ++k) layer[4u * tid + (uint32_t)k] = r.folded.c[k];
                reinterpret_cast<uint4*>(out)[tid] = make_uint4(r.folded.c[0], r.folded.c[1], r.folded.c[2], r.folded.c[3]);
                d = r.leaf;
            } else {
                FoldArgs f{};
                f.dom = a.dom;
                f.coef = mont_mul(transcript_factor(beta[0], a.half_r2), xinvR);   // Montgomery form of beta / (2 x)
                const uint32_t r = fold_one(f, (uint64_t)(tid << shift), layer[tid], layer[tid + half]);
                layer[tid] = r;
                out[tid] = r;
                if (salted) d = merkle_leaf(r, sw);
                else d = merkle_leaf(r, nullptr);
            }
            lvl[tid] = d;
            levels[tid] = d;
        }
        __syncthreads();   // the leaves, and the folded layer, before anything reads them
        uint32_t n = half;
        Digest* next = levels + half;
        while (n > 1u) {
            const uint32_t up = (n + 1u) / 2u;
            const bool active = pair * 64u < up;               // wave-uniform
            const uint32_t i0 = pair * 64u + lane;
            const uint32_t i = i0 < up ? i0 : up - 1u;
            Digest l{}, r{};
            if (active) {
                l = lvl[2u * i];
                r = (2u * i + 1u < n) ? lvl[2u * i + 1u] : l;
            }
            const Digest d = merkle_node_coop(l, r, sched[pair], lane, helper, active);   // its first barrier: every read of the old level is done
            if (active && !helper && i0 < up) {
                lvl[i0] = d;
                next[i0] = d;
            }
            TOYNI_LDS_BARRIER();
            next += up;
            n = up;
        }
        levels += 2u * half - 1u;
        out += half * W;
        if (salted) salts += half;
        if (betas) betas += NSQ;
        xinvR = mont_mul(xinvR, xinvR);   // the squared domain of the next layer
        ++shift;
        m = half;
        have_root = true;
    }
    if (tid == 0u && have_root) transcript_absorb(tr, reinterpret_cast<const uint8_t*>(&lvl[0]), 32u);
    __syncthreads();
    for (uint32_t i = tid; i < TRANSCRIPT_CAPACITY; i += blockDim.x) a.tr->bytes[i] = tr.bytes[i];
    if (tid == 0) { a.tr->len = tr.len; a.tr->status = tr.status; }
}

// ---- a batch dimension for the latency-bound tail (include/toyni_hip.h 3r) ----
// Batch twins of the kernels above: the same launches, each working on `batch` independent proofs that lie a stride apart.  Proof b
// writes exactly what the single kernel writes when given proof b's pointers.  The proof index is a BLOCK coordinate: blockIdx.x where
// one block is one proof (the one-wave and the one-workgroup kernels), blockIdx.y for the sweeps, whose blockIdx.x / gridDim.x keep
// their meaning.  The twins are written out instead of sharing bodies with the originals, so that the originals' code -- registers,
// LDS, occupancy -- cannot move.  Every offset is 64-bit.
__global__ void __launch_bounds__(256) merkle_leaf_batch_kernel(const uint32_t* __restrict__ values0, size_t value_stride, const uint8_t* __restrict__ salts0,
                                                                 size_t salt_stride, uint8_t* __restrict__ levels0, size_t level_stride, size_t n) {
    const size_t b = blockIdx.y;   // the proof: a block coordinate, the same in every lane of every wave of the workgroup
    const uint32_t* values = values0 + b * value_stride;
    const uint4* salts = salts0 ? reinterpret_cast<const uint4*>(salts0 + b * salt_stride) : nullptr;
    Digest* out = reinterpret_cast<Digest*>(levels0 + b * level_stride);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        Digest d;
        if (salts) {
            const uint4 s = salts[i];
            const uint32_t sw[4] = {s.x, s.y, s.z, s.w};
            d = merkle_leaf(values[i], sw);
        } else {
            d = merkle_leaf(values[i], nullptr);
        }
        out[i] = d;
    }
}
// level `at` (a digest offset inside a proof's tree) of m digests -> the level behind it, in every proof
__global__ void __launch_bounds__(256) merkle_level_batch_kernel(uint8_t* __restrict__ levels0, size_t level_stride, size_t at, size_t m, size_t up) {
    const size_t b = blockIdx.y;   // the proof: a block coordinate, wave-uniform
    const Digest* cur = reinterpret_cast<const Digest*>(levels0 + b * level_stride) + at;
    Digest* next = reinterpret_cast<Digest*>(levels0 + b * level_stride) + at + m;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < up; i += stride) {
        const Digest l = cur[2 * i];
        const Digest r = (2 * i + 1 < m) ? cur[2 * i + 1] : l;  // odd level: duplicate the last node (src/merkle.rs:38-42)
        next[i] = merkle_node(l, r);
    }
}
__global__ void __launch_bounds__(128) merkle_level_coop_batch_kernel(uint8_t* __restrict__ levels0, size_t level_stride, size_t at, size_t m, size_t up) {
    __shared__ uint32_t sched[COOP_SCHED_WORDS];
    const size_t b = blockIdx.y;   // the proof: a block coordinate, wave-uniform -- both barriers of merkle_node_coop are reached by every wave
    const Digest* cur = reinterpret_cast<const Digest*>(levels0 + b * level_stride) + at;
    Digest* next = reinterpret_cast<Digest*>(levels0 + b * level_stride) + at + m;
    const uint32_t lane = threadIdx.x & 63u;
    const bool helper = TOYNI_UNIFORM(threadIdx.x >> 6) != 0;
    const size_t i0 = (size_t)blockIdx.x * 64u + lane;
    const size_t i = i0 < up ? i0 : up - 1;
    const Digest l = cur[2 * i];
    const Digest r = (2 * i + 1 < m) ? cur[2 * i + 1] : l;
    const Digest d = merkle_node_coop(l, r, sched, lane, helper, true);
    if (!helper && i0 < up) next[i0] = d;
}
// one workgroup per proof: every barrier condition below is a function of m, which all proofs share
__global__ void __launch_bounds__(MERKLE_TAIL_T) merkle_tail_batch_kernel(uint8_t* __restrict__ levels0, size_t level_stride, size_t at, uint32_t m) {
    __shared__ Digest lvl[MERKLE_TAIL];
    __shared__ uint32_t sched[MERKLE_TAIL_T / 128][COOP_SCHED_WORDS];
    const size_t b = blockIdx.x;   // the proof: a block coordinate, wave-uniform
    const Digest* cur = reinterpret_cast<const Digest*>(levels0 + b * level_stride) + at;
    Digest* next = reinterpret_cast<Digest*>(levels0 + b * level_stride) + at + m;
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) lvl[i] = cur[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = TOYNI_UNIFORM(threadIdx.x >> 6);
    const uint32_t pair = wave >> 1;
    const bool helper = (wave & 1u) != 0u;
    while (m > 1) {
        const uint32_t up = (m + 1) / 2;
        const bool active = pair * 64u < up;               // wave-uniform
        const uint32_t i0 = pair * 64u + lane;
        const uint32_t i = i0 < up ? i0 : up - 1;
        Digest l{}, r{};
        if (active) {
            l = lvl[2 * i];
            r = (2 * i + 1 < m) ? lvl[2 * i + 1] : l;
        }
        const Digest d = merkle_node_coop(l, r, sched[pair], lane, helper, active);   // its first barrier: every read of the old level is done
        if (active && !helper && i0 < up) {
            lvl[i0] = d;
            next[i0] = d;
        }
        TOYNI_LDS_BARRIER();
        next += up;
        m = up;
    }
}

// one wave per transcript
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_absorb_batch_kernel(TranscriptState* __restrict__ tr, const uint8_t* __restrict__ src,
                                                                                size_t byte_stride, uint32_t n) {
    const size_t b = blockIdx.x;   // the proof: a block coordinate, wave-uniform
    transcript_absorb_wave(tr[b], src + b * byte_stride, n, threadIdx.x, TRANSCRIPT_T);
}
__global__ void __launch_bounds__(TRANSCRIPT_T) transcript_squeeze_indices_batch_kernel(TranscriptState* __restrict__ tr, uint32_t count, uint32_t max,
                                                                                         uint32_t* __restrict__ out, size_t out_stride) {
    __shared__ uint32_t seen[TRANSCRIPT_MAX_INDICES];
    __shared__ uint32_t flag;
    const size_t b = blockIdx.x;   // the proof: a block coordinate, wave-uniform
    const auto any_lane = [](bool hit) {   // as in transcript_squeeze_indices_kernel: one LDS word, a wave's LDS operations in program order
        if (threadIdx.x == 0) flag = 0u;
        TOYNI_WAVE_ORDER();
        if (hit) flag = 1u;
        TOYNI_WAVE_ORDER();
        const uint32_t some = flag;
        TOYNI_WAVE_ORDER();
        return some != 0u;
    };
    transcript_squeeze_indices(tr[b], count, max, out + b * out_stride, seen, threadIdx.x, TRANSCRIPT_T, any_lane);
}
__global__ void __launch_bounds__(256) fri_query_positions_batch_kernel(const uint32_t* __restrict__ indices, size_t index_stride, uint32_t count, uint64_t m0,
                                                                        uint64_t total, uint32_t* __restrict__ out, size_t out_stride) {
    const size_t b = blockIdx.y;   // the proof: a block coordinate, wave-uniform
    const uint32_t* idx = indices + b * index_stride;
    uint32_t* o = out + b * out_stride;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) o[t] = fri_query_position(idx, count, m0, t);
}

// Between two rounds, one wave per proof: proof b absorbs its root, squeezes and leaves its record at rec + b * rec_stride.
__global__ void __launch_bounds__(TRANSCRIPT_T) fri_transcript_round_batch_kernel(TranscriptState* __restrict__ tr0, const uint8_t* __restrict__ root0,
                                                                                   size_t root_stride, uint32_t nsqueeze, uint32_t c0, uint32_t c1,
                                                                                   uint32_t* __restrict__ rec0, uint32_t rec_stride,
                                                                                   uint32_t* __restrict__ betas0, size_t beta_stride) {
    __shared__ uint32_t beta[4];
    const size_t b = blockIdx.x;   // the proof: a block coordinate, wave-uniform; the barrier below hangs on nsqueeze alone
    TranscriptState& tr = tr0[b];
    uint32_t* rec = rec0 + b * rec_stride;
    uint32_t* betas = betas0 ? betas0 + b * beta_stride : nullptr;
    if (threadIdx.x == 0) {
        if (root0) transcript_absorb(tr, root0 + b * root_stride, 32u);
        transcript_squeeze(tr, beta, nsqueeze);
    }
    if (nsqueeze == 0u) return;
    __syncthreads();
    if (threadIdx.x < nsqueeze) {
        const uint32_t v = beta[threadIdx.x];
        if (betas) betas[threadIdx.x] = v;
        rec[threadIdx.x] = transcript_factor(v, c0);
        if (nsqueeze == 4u) rec[4u + threadIdx.x] = transcript_factor(v, c1);
    }
}

// The folds: proof b reads its layer at evals + b * in_stride, writes out + b * out_stride (strides in words), its leaves at
// levels + b * level_stride (bytes), its salts at salts + b * salt_stride (bytes), with the factor of record b.
struct FoldBatch {
    size_t in_stride, out_stride, salt_stride, level_stride;
    uint32_t rec_stride;
};
__global__ void __launch_bounds__(256) fri_fold_commit_rec_batch_kernel(const FoldArgs f0, const FoldBatch st, const uint32_t* __restrict__ rec,
                                                                        const uint8_t* __restrict__ salts0, uint8_t* __restrict__ levels0) {
    const size_t b = blockIdx.y;   // the proof: a block coordinate, wave-uniform
    FoldArgs f = f0;
    f.evals = f0.evals + b * st.in_stride;
    f.out = f0.out + b * st.out_stride;
    f.coef = rec[b * st.rec_stride];
    const uint4* salts = salts0 ? reinterpret_cast<const uint4*>(salts0 + b * st.salt_stride) : nullptr;
    Digest* leaves = reinterpret_cast<Digest*>(levels0 + b * st.level_stride);
    const uint64_t half = f.half;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += stride) {
        const uint32_t r = fold_one(f, i, f.evals[i], f.evals[i + half]);
        f.out[i] = r;
        if (salts) {
            const uint4 sv = salts[i];
            const uint32_t sw[4] = {sv.x, sv.y, sv.z, sv.w};
            leaves[i] = merkle_leaf(r, sw);
        } else {
            leaves[i] = merkle_leaf(r, nullptr);
        }
    }
}
template <bool SALTED>
__global__ void __launch_bounds__(256) fri_fold_ext_commit_rec_batch_kernel(const FoldArgs f, const FoldBatch st, const uint32_t* __restrict__ rec,
                                                                            const uint8_t* __restrict__ salts0, uint8_t* __restrict__ levels0) {
    const size_t b = blockIdx.y;   // the proof: a block coordinate, wave-uniform
    const ExtFactor beta_half = *reinterpret_cast<const ExtFactor*>(rec + b * st.rec_stride);
    const uint64_t half = f.half;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint4* ea = reinterpret_cast<const uint4*>(f.evals + b * st.in_stride);
    const uint4* eb = ea + half;
    uint4* o = reinterpret_cast<uint4*>(f.out + b * st.out_stride);
    const uint4* salts = reinterpret_cast<const uint4*>(salts0 + (SALTED ? b * st.salt_stride : 0));
    Digest* leaves = reinterpret_cast<Digest*>(levels0 + b * st.level_stride);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < half; i += stride) {
        const uint32_t scaleR = mont_mul(subdomain_mont(f.dom, (uint32_t)i), f.coef);
        const uint4 a = ea[i], c = eb[i];
        uint32_t sw[4] = {0u, 0u, 0u, 0u};
        if constexpr (SALTED) {
            const uint4 s = salts[i];
            sw[0] = s.x; sw[1] = s.y; sw[2] = s.z; sw[3] = s.w;
        }
        const FoldExtLeaf r = fold_ext_commit_one<SALTED>(Ext4{{a.x, a.y, a.z, a.w}}, Ext4{{c.x, c.y, c.z, c.w}}, scaleR, beta_half, sw);
        o[i] = make_uint4(r.folded.c[0], r.folded.c[1], r.folded.c[2], r.folded.c[3]);
        leaves[i] = r.leaf;
    }
}

// fri_tail_rounds_kernel, one workgroup per proof.  The proof index only moves the six pointers; m, final_size and with them every
// loop count and every barrier condition are shared by all proofs of the launch, so each workgroup runs the original's barrier
// sequence.  a.cur, a.out, a.levels, a.salts, a.betas and a.tr are proof 0's; a null a.salts / a.betas is null for every proof.
struct FriTailBatch { size_t cur_stride, out_stride, level_stride, salt_stride, beta_stride; };   // words, words, bytes, bytes, words
template <bool EXT>
__global__ void __launch_bounds__(MERKLE_TAIL_T) fri_tail_rounds_batch_kernel(const FriTailArgs a, const FriTailBatch st) {
    constexpr uint32_t W = EXT ? 4u : 1u, NSQ = EXT ? 4u : 1u;
    __shared__ uint32_t layer[2 * MERKLE_TAIL * W];
    __shared__ Digest lvl[MERKLE_TAIL];
    __shared__ uint32_t sched[MERKLE_TAIL_T / 128][COOP_SCHED_WORDS];
    __shared__ TranscriptState tr;
    __shared__ uint32_t beta[4];
    const size_t b = blockIdx.x;   // the proof: a block coordinate, the same in every wave -- the barriers below depend on m alone
    const uint32_t* in = a.cur + b * st.cur_stride;
    TranscriptState* gtr = a.tr + b;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = TOYNI_UNIFORM(tid >> 6);
    const uint32_t pair = wave >> 1;
    const bool helper = (wave & 1u) != 0u;
    for (uint32_t i = tid; i < a.m * W; i += blockDim.x) layer[i] = in[i];
    for (uint32_t i = tid; i < TRANSCRIPT_CAPACITY; i += blockDim.x) tr.bytes[i] = gtr->bytes[i];
    if (tid == 0) { tr.len = gtr->len; tr.status = gtr->status; }
    __syncthreads();
    uint32_t m = a.m, shift = 0, xinvR = a.xinvR;
    uint32_t* out = a.out + b * st.out_stride;
    Digest* levels = reinterpret_cast<Digest*>(reinterpret_cast<uint8_t*>(a.levels) + b * st.level_stride);
    const uint4* salts = a.salts ? reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(a.salts) + b * st.salt_stride) : nullptr;
    uint32_t* betas = a.betas ? a.betas + b * st.beta_stride : nullptr;
    bool have_root = false;
    while (m > a.final_size) {
        const uint32_t half = m >> 1;
        const bool salted = salts && half != a.final_size;
        if (tid == 0u) {
            if (have_root) transcript_absorb(tr, reinterpret_cast<const uint8_t*>(&lvl[0]), 32u);
            transcript_squeeze(tr, beta, NSQ);
            if (betas) {
#pragma unroll
                for (uint32_t k = 0; k < NSQ; ++k) betas[k] = beta[k];
            }
        }
        __syncthreads();   // beta is there; the root has been read before a leaf of this round replaces it
        if (tid < half) {
            uint32_t sw[4] = {0u, 0u, 0u, 0u};
            if (salted) {
                const uint4 sv = salts[tid];
                sw[0] = sv.x; sw[1] = sv.y; sw[2] = sv.z; sw[3] = sv.w;
            }
            Digest d;
            if constexpr (EXT) {
                ExtFactor f;
#pragma unroll
                for (int k = 0; k < 4; ++k) { f.b[k] = transcript_factor(beta[k], a.half_r2); f.b11[k] = transcript_factor(beta[k], a.half11_r2); }
                const uint32_t scaleR = mont_mul(subdomain_mont(a.dom, tid << shift), xinvR);
                const uint32_t* pa = layer + 4u * tid;
                const uint32_t* pb = layer + 4u * (tid + half);
                const Ext4 va{{pa[0], pa[1], pa[2], pa[3]}}, vb{{pb[0], pb[1], pb[2], pb[3]}};
                const FoldExtLeaf r = salted ? fold_ext_commit_one<true>(va, vb, scaleR, f, sw) : fold_ext_commit_one<false>(va, vb, scaleR, f, sw);
#pragma unroll
                for (int k = 0; k < 4; ++k) layer[4u * tid + (uint32_t)k] = r.folded.c[k];
                reinterpret_cast<uint4*>(out)[tid] = make_uint4(r.folded.c[0], r.folded.c[1], r.folded.c[2], r.folded.c[3]);
                d = r.leaf;
            } else {
                FoldArgs f{};
                f.dom = a.dom;
                f.coef = mont_mul(transcript_factor(beta[0], a.half_r2), xinvR);   // Montgomery form of beta / (2 x)
                const uint32_t r = fold_one(f, (uint64_t)(tid << shift), layer[tid], layer[tid + half]);
                layer[tid] = r;
                out[tid] = r;
                if (salted) d = merkle_leaf(r, sw);
                else d = merkle_leaf(r, nullptr);
            }
            lvl[tid] = d;
            levels[tid] = d;
        }
        __syncthreads();   // the leaves, and the folded layer, before anything reads them
        uint32_t n = half;
        Digest* next = levels + half;
        while (n > 1u) {
            const uint32_t up = (n + 1u) / 2u;
            const bool active = pair * 64u < up;               // wave-uniform
            const uint32_t i0 = pair * 64u + lane;
            const uint32_t i = i0 < up ? i0 : up - 1u;
            Digest l{}, r{};
            if (active) {
                l = lvl[2u * i];
                r = (2u * i + 1u < n) ? lvl[2u * i + 1u] : l;
            }
            const Digest d = merkle_node_coop(l, r, sched[pair], lane, helper, active);   // its first barrier: every read of the old level is done
            if (active && !helper && i0 < up) {
                lvl[i0] = d;
                next[i0] = d;
            }
            TOYNI_LDS_BARRIER();
            next += up;
            n = up;
        }
        levels += 2u * half - 1u;
        out += half * W;
        if (salted) salts += half;
        if (betas) betas += NSQ;
        xinvR = mont_mul(xinvR, xinvR);   // the squared domain of the next layer
        ++shift;
        m = half;
        have_root = true;
    }
    if (tid == 0u && have_root) transcript_absorb(tr, reinterpret_cast<const uint8_t*>(&lvl[0]), 32u);
    __syncthreads();
    for (uint32_t i = tid; i < TRANSCRIPT_CAPACITY; i += blockDim.x) gtr->bytes[i] = tr.bytes[i];
    if (tid == 0) { gtr->len = tr.len; gtr->status = tr.status; }
}

#ifndef TOYNI_KERNEL_TEXT_ONLY
// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct ShiftTable {
    uint32_t* d = nullptr;  // two-level power tables of shift (dir 0) and shift^-1 (dir 1)
    uint32_t lo_off[2], hi_off[2], lowbits;
    uint32_t s[2];
};

struct toyni_ntt_ctx {
    NttPlan plan;
    // n = 2^21 / 2^22 only: a second, two-pass plan (2048-point three-step shapes) for launches of one or two transforms
    NttPlan plan_lat;
    bool has_lat = false;
    uint32_t* d_fwd_lat = nullptr;
    uint32_t* d_inv_lat = nullptr;
    uint32_t n = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t* d_fwd = nullptr;
    uint32_t* d_inv = nullptr;
    // Intermediates (the reference keeps ONE shared NttCtx::d_data, cuda/ntt_kernel.cu:205 -- the race of SURVEY.md F8).
    // Here every stream that carries calls of this context has its own set, so calls enqueued on different streams
    // never share a buffer and calls on one stream are ordered by the stream: no cross-stream hazard, nothing to wait for.
    struct Scratch {
        uint32_t* d_work = nullptr;      // intermediate of multi-pass transforms
        size_t work_words = 0;
        uint32_t* d_data32 = nullptr;    // packed copy for the host / u64 / Ext entry points
        size_t data32_words = 0;
        uint64_t* d_stage64 = nullptr;   // H2D / D2H staging on the reference's u64 layout
        size_t stage64_elems = 0;
        uint32_t* d_lde32 = nullptr;     // compact coefficient vectors of the LDE entry points
        size_t lde32_words = 0;
        uint32_t* d_fri_rec = nullptr;   // the per-round beta records of the transcript commit phases (3l): FRI_REC_WORDS words, fixed
        size_t fri_rec_words = 0;
        uint8_t* h_ring = nullptr;       // pinned staging ring: host tables that a stream-ordered copy reads after the call returned
        size_t ring_bytes = 0, ring_head = 0;
        uint64_t tick = 0;               // last use (eviction order)
        hipEvent_t fence = nullptr;      // recorded on the set's stream at the end of the last call that used it (when `fenced`)
        bool fenced = false;             // `fence` covers every use of the set so far
        bool dirty = false;              // used by the call in progress (finish_call records the fence)
    };
    std::map<hipStream_t, Scratch> scratch;
    uint64_t tick = 0;
    // Buffers that were outgrown or evicted.  They may still be read by kernels in flight, and hipFree is a device-wide
    // synchronisation, so nothing is freed on an enqueue path: a retired buffer is freed after a synchronisation of the
    // stream it belonged to (blocking host entry points, toyni_stream_synchronize), by toyni_ntt_ctx_trim, or at destroy.
    // Round 3: a retired buffer that has an EVENT (recorded on its stream after its last possible use) is freed by the next
    // call on this context that finds the event complete -- so a caller that cycles through short-lived streams, or grows its
    // batch on a stream it never synchronises through this API, no longer accumulates buffers until trim.
    struct Retired { void* ptr; hipStream_t stream; bool stream_known; hipEvent_t ev; bool fresh; };
    std::vector<Retired> retired;
    size_t chunk_elems = 0;          // 0 = whole batch in one launch sequence
    int num_cus = 256;
    std::map<uint32_t, ShiftTable> shifts;
    // Pipelined host-slice path for callers that hand over PINNED host memory (toyni_host_alloc / hipHostRegister): two
    // staging slots, a copy-in and a copy-out stream next to the compute stream, so that the upload of chunk k + 1, the
    // kernels of chunk k and the download of chunk k - 1 overlap (PCIe is full duplex).
    struct HostPipe {
        hipStream_t in = nullptr, out = nullptr;
        hipEvent_t in_done[2] = {nullptr, nullptr}, comp_done[2] = {nullptr, nullptr}, out_done[2] = {nullptr, nullptr};
        uint64_t* d_stage[2] = {nullptr, nullptr};
        uint32_t* d_data[2] = {nullptr, nullptr};
        size_t cap_elems = 0;
        bool ready = false;
    } pipe;
#ifdef TOYNI_TOOLS                  // measurement build only (libtoyni_hip_tools.so, include/toyni_hip_tools.h)
    struct TimingRec { hipEvent_t e0, e1; int dir, pass; };
    bool timing = false;             // toyni_ntt_ctx_timing: bracket every pass launch with events
    std::vector<TimingRec> timing_recs;
#endif
    uint8_t* h_root = nullptr;       // pinned: the per-round root of toyni_fri_commit_phase_device (32 bytes + a sequence word the
    uint32_t* d_root_notify = nullptr;  // tree's last kernel stores through this device alias of the same memory)
    uint32_t root_seq = 0;
    uint32_t* d_ones = nullptr;      // Montgomery ones: the twiddle-free closing pass of a multi-device inverse (slab_pass)
    std::mutex mu;
};

namespace {

// The context whose transcript callback (toyni_fri_commit_phase_device) is running on THIS thread, if any.  The callback runs with
// the context locked, so an entry point on the same context from inside it would deadlock on c->mu; it returns
// TOYNI_E_REENTRANT instead (the rule was documented but not enforced).
// (round 4, ADVICE r3: a STACK, not one slot -- a callback of context A may run a commit phase on context B, whose own callbacks push
// and pop B; A must still be refused afterwards.)
thread_local std::vector<const toyni_ntt_ctx*> t_callback_ctxs;
inline bool in_callback_of(const toyni_ntt_ctx* c) {
    for (const toyni_ntt_ctx* x : t_callback_ctxs)
        if (x == c) return true;
    return false;
}
struct CallbackScope {
    explicit CallbackScope(const toyni_ntt_ctx* c) { t_callback_ctxs.push_back(c); }
    ~CallbackScope() { t_callback_ctxs.pop_back(); }
};
void finish_call(toyni_ntt_ctx* c);
struct CtxCall {   // declared right after the lock: destroyed before it is released
    toyni_ntt_ctx* c;
    ~CtxCall() { finish_call(c); }
};
#define TOYNI_CTX_LOCK(c)                                   \
    if (in_callback_of(c)) return TOYNI_E_REENTRANT;       \
    std::lock_guard<std::mutex> lk((c)->mu);               \
    CtxCall _ctx_call{(c)}

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

constexpr size_t MAX_SCRATCH_STREAMS = 8;

// Fencing policy (TOYNI_FENCE = auto | always | never; read once).  A fence is one hipEventRecord at the end of a call, on every
// stream whose scratch set the call used.  auto (default): while the context serves more than one stream, and for any set that
// holds >= 64 MiB -- so a lone small transform on a single stream (the latency path) records nothing.  The one hole of `auto`: a
// SMALL set of the first stream, last used before a second stream appeared, is unfenced; evicted, it waits for trim like in
// round 2 (at most one set of < 64 MiB per context).
int fence_mode() {
    static const int v = [] {
        const char* e = std::getenv("TOYNI_FENCE");
        if (e && !std::strcmp(e, "always")) return 2;
        if (e && !std::strcmp(e, "never")) return 0;
        return 1;
    }();
    return v;
}

void retire_scratch(toyni_ntt_ctx* c, toyni_ntt_ctx::Scratch& sc, hipStream_t s, bool stream_known) {
    // an evicted set's stream may no longer exist, so nothing can be recorded on it now: the set's own fence, recorded when the
    // stream was last used, is what lets its buffers go (one event shared by the set's buffers: the last one to go destroys it)
    hipEvent_t ev = (sc.fenced && !sc.dirty) ? sc.fence : nullptr;
    bool handed = false;
    for (void* p : {(void*)sc.d_work, (void*)sc.d_data32, (void*)sc.d_stage64, (void*)sc.d_lde32, (void*)sc.d_fri_rec})
        if (p) { c->retired.push_back({p, s, stream_known, ev, false}); handed = true; }
    if (sc.fence && !(ev && handed)) (void)hipEventDestroy(sc.fence);
    if (sc.h_ring) (void)hipHostFree(sc.h_ring);   // waits for the copies that still read it (eviction, trim, destroy: never the steady state)
    sc = toyni_ntt_ctx::Scratch();
}

// the scratch set of stream s (caller holds c->mu).  At most MAX_SCRATCH_STREAMS sets are kept: the least recently used
// one is retired (its stream may no longer exist, so those buffers wait for toyni_ntt_ctx_trim / destroy).
toyni_ntt_ctx::Scratch& scratch_for(toyni_ntt_ctx* c, hipStream_t s) {
    auto it = c->scratch.find(s);
    if (it == c->scratch.end()) {
        if (c->scratch.size() >= MAX_SCRATCH_STREAMS) {
            auto lru = c->scratch.begin();
            for (auto j = c->scratch.begin(); j != c->scratch.end(); ++j)
                if (j->first != c->stream && (lru->first == c->stream || j->second.tick < lru->second.tick)) lru = j;
            retire_scratch(c, lru->second, lru->first, false);
            c->scratch.erase(lru);
        }
        it = c->scratch.emplace(s, toyni_ntt_ctx::Scratch()).first;
    }
    it->second.tick = ++c->tick;
    it->second.dirty = true;
    return it->second;
}

// grow-only; the outgrown buffer is retired, not freed (no hipFree -- a device-wide sync -- on an enqueue path)
int grow(toyni_ntt_ctx* c, hipStream_t s, void** buf, size_t* have, size_t need, size_t elem_bytes) {
    if (*have >= need) return 0;
    if (*buf) { c->retired.push_back({*buf, s, true, nullptr, true}); *buf = nullptr; *have = 0; }   // fresh: finish_call fences it on s
    HIPCHK(hipMalloc(buf, need * elem_bytes));
    *have = need;
    return 0;
}

// `bytes` of the set's pinned staging ring.  Slices are handed out in order; before the ring wraps or is replaced by a larger one the
// stream is drained, so no slice is rewritten while an enqueued copy may still read it (once per 64 KiB of tables at the least).
int ring_slice(toyni_ntt_ctx::Scratch& sc, hipStream_t s, size_t bytes, void** out) {
    bytes = (bytes + 63) & ~(size_t)63;
    if (sc.ring_head + bytes > sc.ring_bytes) {
        HIPCHK(hipStreamSynchronize(s));
        sc.ring_head = 0;
        if (bytes > sc.ring_bytes) {
            if (sc.h_ring) { (void)hipHostFree(sc.h_ring); sc.h_ring = nullptr; sc.ring_bytes = 0; }
            const size_t want = std::max<size_t>(bytes, (size_t)64 << 10);
            HIPCHK(hipHostMalloc((void**)&sc.h_ring, want, hipHostMallocDefault));
            sc.ring_bytes = want;
        }
    }
    *out = sc.h_ring + sc.ring_head;
    sc.ring_head += bytes;
    return 0;
}

// after stream s has been synchronised by the caller: nothing enqueued on it can still touch what it retired
// several retired buffers may share one event (an evicted set): it is destroyed with the last of them
void drop_retired_event(toyni_ntt_ctx* c, size_t index) {
    hipEvent_t ev = c->retired[index].ev;
    if (!ev) return;
    c->retired[index].ev = nullptr;   // this entry no longer holds it: when all sharers go in one sweep, the last one still destroys it
    for (size_t j = 0; j < c->retired.size(); ++j)
        if (c->retired[j].ev == ev) return;
    (void)hipEventDestroy(ev);
}

void reclaim_after_sync(toyni_ntt_ctx* c, hipStream_t s) {
    size_t keep = 0;
    for (size_t i = 0; i < c->retired.size(); ++i) {
        auto& r = c->retired[i];
        if (r.stream_known && r.stream == s) { (void)hipFree(r.ptr); r.ptr = nullptr; }
    }
    for (size_t i = 0; i < c->retired.size(); ++i)
        if (!c->retired[i].ptr) drop_retired_event(c, i);
    for (auto& r : c->retired)
        if (r.ptr) c->retired[keep++] = r;
    c->retired.resize(keep);
}

// End of every call on a context (TOYNI_CTX_LOCK's guard; the context is still locked): fence what the call used, then free the
// retired buffers whose fence has completed.  Steady state (one stream, nothing retired): two empty loops.
void finish_call(toyni_ntt_ctx* c) {
    bool fresh = false;
    for (auto& r : c->retired) fresh |= r.fresh;
    const int mode = fence_mode();
    const bool fence_sets = mode == 2 || (mode == 1 && c->scratch.size() > 1);
    bool any_dirty = false;
    for (auto& kv : c->scratch) any_dirty |= kv.second.dirty;
    if (!any_dirty && !fresh && c->retired.empty()) return;
    DeviceGuard guard(c->device);
    // streams KNOWN to be alive: the ones this very call enqueued on, and the context's own.  Only those are asked whether they are
    // capturing below -- a key of c->scratch may be a stream its owner has destroyed since (querying a stale handle is
    // undefined, and a recycled handle could block the sweep for ever or wrongly allow it)
    hipStream_t live[MAX_SCRATCH_STREAMS + 1];
    size_t nlive = 0;
    live[nlive++] = c->stream;
    for (auto& kv : c->scratch) {
        toyni_ntt_ctx::Scratch& sc = kv.second;
        if (!sc.dirty) continue;
        if (kv.first != c->stream && nlive < MAX_SCRATCH_STREAMS + 1) live[nlive++] = kv.first;
        sc.dirty = false;
        sc.fenced = false;
        // a set that holds real memory is fenced in single-stream use too: its calls are long (the event is noise next to them) and
        // an unfenced eviction would pin that memory until trim; small sets (lone transforms: the latency path) stay event-free
        const size_t set_bytes = sc.work_words * 4 + sc.data32_words * 4 + sc.stage64_elems * 8 + sc.lde32_words * 4;
        bool need = fence_sets || set_bytes >= ((size_t)64 << 20);
        for (auto& r : c->retired) need |= r.fresh && r.stream == kv.first;
        if (!need || mode == 0) continue;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(kv.first, &cap) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (cap != hipStreamCaptureStatusNone) continue;        // a captured call leaves no fence: replays are not this call
        if (!sc.fence && hipEventCreateWithFlags(&sc.fence, hipEventDisableTiming) != hipSuccess) { sc.fence = nullptr; (void)hipGetLastError(); continue; }
        if (hipEventRecord(sc.fence, kv.first) != hipSuccess) { (void)hipGetLastError(); continue; }
        sc.fenced = true;
        // what this call outgrew on this stream: everything enqueued before the fence is the last that can touch it.  The buffer
        // gets an event of its own (the set's fence moves on with the next call).
        for (auto& r : c->retired) {
            if (!(r.fresh && r.stream == kv.first)) continue;
            hipEvent_t ev = nullptr;
            if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, kv.first) == hipSuccess) r.ev = ev;
            else { if (ev) (void)hipEventDestroy(ev); (void)hipGetLastError(); }
        }
    }
    for (auto& r : c->retired) r.fresh = false;
    // free what has drained.  hipFree synchronises the device, which is why nothing is freed on the enqueue path of a steady-state
    // caller -- but there IS nothing to free there; this runs only after an eviction or an outgrown buffer.  Relaxed capture mode:
    // a hipFree must not invalidate a capture this thread has open on some stream.
    bool any_ready = false;
    for (auto& r : c->retired)
        if (r.ev && hipEventQuery(r.ev) == hipSuccess) { any_ready = true; break; }
    (void)hipGetLastError();   // hipErrorNotReady from the queries is not an error
    if (!any_ready) return;
    // hipFree synchronises the device and is illegal while a global-mode capture is open.  Relaxed mode below covers THIS thread; a
    // capture open on a stream THIS call used (or on the context's own stream) is visible here, and then the sweep waits for a later
    // call.  What cannot be seen -- a global-mode capture on any other stream -- is the caveat documented in
    // include/toyni_hip.h: capture with hipStreamCaptureModeThreadLocal / Relaxed, or call toyni_ntt_ctx_trim first.
    for (size_t i = 0; i < nlive; ++i) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(live[i], &cap) != hipSuccess) { (void)hipGetLastError(); continue; }
        if (cap != hipStreamCaptureStatusNone) return;
    }
    hipStreamCaptureMode cmode = hipStreamCaptureModeRelaxed;
    (void)hipThreadExchangeStreamCaptureMode(&cmode);
    for (size_t i = 0; i < c->retired.size(); ++i) {
        auto& r = c->retired[i];
        if (r.ev && hipEventQuery(r.ev) == hipSuccess) { (void)hipFree(r.ptr); r.ptr = nullptr; }
    }
    (void)hipGetLastError();
    (void)hipThreadExchangeStreamCaptureMode(&cmode);
    for (size_t i = 0; i < c->retired.size(); ++i)
        if (!c->retired[i].ptr) drop_retired_event(c, i);
    size_t keep = 0;
    for (auto& r : c->retired)
        if (r.ptr) c->retired[keep++] = r;
    c->retired.resize(keep);
}

int grid_for(size_t items, int block = 256) {
    size_t g = (items + block - 1) / block;
    const size_t cap = 256 * 8;  // 8 workgroups per CU, grid-stride beyond
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// prefetch depth of the interleaved (Ext) shapes: the prefetching kernel, except the single-pass 1024-point shape (32 virtual rows
// per tile: with the next tile's 32 loads in flight it needs 128 VGPRs + 100 B of scratch; without them it fits)
template <class P> constexpr int ext_prefetch() { return (kind_of<P>() == KIND_ROW_N && P::LM == 10) ? 0 : 32; }

// The shapes whose kernel reads PassArgs::seeds_invariant: the two-step column shapes of ntt_pass_kernel.  Not their pieces-layout
// variants (the flag costs those six SGPRs and with them a wave of occupancy; one rank's launches are a few tiles per workgroup),
// and not the streaming 2048-point column shape of ntt_pass3s_kernel: its five seed registers, live across the loop, put the
// blow-up-2 variant at 128 VGPRs + 16 B of scratch.
template <class P> constexpr bool hoists_seeds() {
    if constexpr (P::STEPS == 2) return kind_of<P>() == KIND_COL && !P::SLAB;
    else return false;
}

template <class P> constexpr uint32_t log_tile_width() {
    uint32_t l = 0;
    while ((1u << l) < P::C) ++l;
    return l;
}

template <class P, int LZ = 0>
void launch_pass(unsigned grid, hipStream_t s, const PassArgs& args, uint32_t ntiles) {
    PassArgs a = args;
    if constexpr (hoists_seeds<P>()) a.seeds_invariant = seeds_launch_invariant(grid, ntiles, a.log_S, log_tile_width<P>()) ? 1u : 0u;
    if constexpr (P::STEPS == 3) {
        if constexpr (P::STREAM) hipLaunchKernelGGL((ntt_pass3s_kernel<P, LZ>), dim3(grid), dim3(P::T), 0, s, a, ntiles);
        else hipLaunchKernelGGL((ntt_pass3_kernel<P, LZ>), dim3(grid), dim3(P::T), 0, s, a, ntiles);
    } else if constexpr (LZ > 0) {  // LDE first pass: one kernel each
        hipLaunchKernelGGL((ntt_pass_kernel<P, 32, LZ>), dim3(grid), dim3(P::T), 0, s, a, ntiles);
    } else if constexpr (P::LQ > 0) {  // interleaved (Ext) shapes: one kernel each (no A/B twin)
        hipLaunchKernelGGL((ntt_pass_kernel<P, ext_prefetch<P>()>), dim3(grid), dim3(P::T), 0, s, a, ntiles);
    } else {
        // (rounds 1-3 kept a no-prefetch twin of every shape instantiated: removing it once made the prefetching kernel spill.  With
        // today's bodies it does not -- identical VGPR counts within one register, no scratch, and the same throughput in an alternating
        // A/B at 2^14 ... 2^24, profiles/r04_ab_notwins.txt -- so the twins and their TOYNI_PREFETCH knob are gone: 55 kernels fewer)
        hipLaunchKernelGGL((ntt_pass_kernel<P, 32>), dim3(grid), dim3(P::T), 0, s, a, ntiles);
    }
}

// Grid of a persistent pass launch: every CU gets as many workgroups as fit (LDS / registers), capped by the tile
// count; TOYNI_WG_PER_CU overrides the occupancy query (tuning knob).
// (LZ: the zero-fraction variant that will be launched -- only the streaming three-step shapes ask about that very instantiation, so
// that no variant exists in the binary merely because its occupancy was queried)
template <class P, int LZ = 0>
unsigned persistent_grid(toyni_ntt_ctx* c, uint64_t ntiles) {
    static const int per_cu = [] {  // once per instantiation (thread-safe initialisation)
        int occ = 0;
        hipError_t qe;
        if constexpr (P::STEPS == 3) {
            if constexpr (P::STREAM) qe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ntt_pass3s_kernel<P, LZ>, (int)P::T, 0);
            else qe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ntt_pass3_kernel<P, 0>, (int)P::T, 0);
        } else if constexpr (P::LQ > 0) qe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ntt_pass_kernel<P, ext_prefetch<P>()>, (int)P::T, 0);
        else qe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ntt_pass_kernel<P, 32>, (int)P::T, 0);
        if (qe != hipSuccess || occ < 1) occ = 1;
        if (const int v = env_int("TOYNI_WG_PER_CU", 0); v > 0) occ = v;
        return occ;
    }();
    uint64_t g = (uint64_t)c->num_cus * (uint64_t)per_cu;
    if (g > ntiles) g = ntiles;
    if (g >= 16) g &= ~(uint64_t)15;  // keep the XCD pairing of tile_order aligned across loop iterations
    return (unsigned)(g < 1 ? 1 : g);
}

// Measurement build (-DTOYNI_TOOLS, libtoyni_hip_tools.so): every pass launch of a context whose timing switch is on is
// bracketed by a pair of HIP events on the launch stream.  The shipped library compiles these hooks to nothing.
#ifdef TOYNI_TOOLS
struct PassTimer {
    toyni_ntt_ctx* c;
    hipStream_t s;
    toyni_ntt_ctx::TimingRec rec;
    bool on;
    PassTimer(toyni_ntt_ctx* c_, hipStream_t s_, int dir, int pass) : c(c_), s(s_), rec{nullptr, nullptr, dir, pass}, on(false) {
        if (!c->timing) return;
        if (hipEventCreate(&rec.e0) != hipSuccess) return;
        if (hipEventCreate(&rec.e1) != hipSuccess) { (void)hipEventDestroy(rec.e0); return; }
        (void)hipEventRecord(rec.e0, s);
        on = true;
    }
    ~PassTimer() {
        if (!on) return;
        (void)hipEventRecord(rec.e1, s);
        c->timing_recs.push_back(rec);
    }
};
#define TOYNI_PASS_TIMER(c, s, dir, pass) PassTimer _pass_timer((c), (s), (dir), (pass))
#else
#define TOYNI_PASS_TIMER(c, s, dir, pass) ((void)0)
#endif

int get_shift_table(toyni_ntt_ctx* c, uint32_t shift, ShiftTable** out);

// the launch route (ntt_route.hpp) of `batch` transforms (lq = 2: Ext vectors) on this context, under the process's knobs
Route route_of(const toyni_ntt_ctx* c, uint64_t batch, int lq = 0, int log_blowup = 0) {
    return route_transform(c->plan, c->has_lat ? &c->plan_lat : nullptr, batch, lq, log_blowup, c->chunk_elems, launch_knobs());
}

// Enqueue the passes of ONE launch sequence (for_each_pass) on stream s, each as a persistent launch (bracketed by the measurement
// build's timer).  TOYNI_E_INVALID_SIZE when the plan has no shape for a pass, else the first HIP error.
template <int LQ>
int run_passes(toyni_ntt_ctx* c, const NttPlan& plan, const uint32_t* tables, bool inverse, const uint32_t* src, uint32_t* work, uint32_t* dst,
               uint64_t batch, hipStream_t s, const CosetTables& cs = CosetTables(), int lde_log = 0, bool nt = false, const SlabIo* sio = nullptr) {
    hipError_t err = hipSuccess;
    int pass_index = 0;
    const bool ok = for_each_pass<LQ>(launch_knobs(), plan, tables, inverse, src, work, dst, batch, [&](auto pass, auto lzc, const PassArgs& a, uint64_t nblocks) {
        using P = decltype(pass);
        constexpr int LZ = decltype(lzc)::value;
        const int p = pass_index++;
        if (err != hipSuccess) return;
        TOYNI_PASS_TIMER(c, s, inverse ? 1 : 0, p);
        launch_pass<P, LZ>(persistent_grid<P, LZ>(c, nblocks), s, a, (uint32_t)nblocks);
        err = hipGetLastError();
    }, cs, lde_log, nt, sio);
    return ok ? (int)err : TOYNI_E_INVALID_SIZE;
}

// Enqueue `batch` transforms on stream s (d_in == d_out allowed), by the route of ntt_route.hpp.  shift != 1: the coset scaling of
// BabyBearDomain::fft / ifft is fused into the first / last pass.
// log_blowup > 0 (forward only, d_in != d_out): the low-degree extension (src/fibonacci.rs:101-103 / BabyBearDomain::fft on a coefficient
// vector shorter than the domain, src/math/domain.rs:107-123) -- d_in holds the n >> log_blowup leading words of every transform.  Where the
// route fuses it, the padding is never materialised: the first pass reads the words that exist and skips the butterflies whose partner is zero.
// lq = 2: `batch` Ext vectors in the reference's AoS layout ([n][4] words each; log_blowup > 0: [n >> log_blowup][4] in): the interleaved
// variants of the same passes (Pass<..., LQ = 2>), i.e. fft_ext / ifft_ext (src/math/domain.rs:129-151) without a de-interleave.
int enqueue_transform(toyni_ntt_ctx* c, const uint32_t* d_in, uint32_t* d_out, size_t batch, bool inverse, hipStream_t s, uint32_t shift = 1u,
                      int log_blowup = 0, int lq = 0) {
    if (batch == 0) return 0;
    const Route r = route_of(c, batch, lq, log_blowup);
    if (r.pad) {   // materialise the padding, transform in place
        const size_t nw = (size_t)c->n << lq, nw_in = nw >> log_blowup;   // words per vector
        HIPCHK(hipMemsetAsync(d_out, 0, batch * nw * sizeof(uint32_t), s));
        HIPCHK(hipMemcpy2DAsync(d_out, nw * sizeof(uint32_t), d_in, nw_in * sizeof(uint32_t), nw_in * sizeof(uint32_t), batch, hipMemcpyDeviceToDevice, s));
        d_in = d_out;
    }
    batch <<= lq;   // from here on in base-field transforms (Q interleaved ones per Ext vector)
    const size_t n = c->n;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    const size_t n_in = n >> r.lde_log;  // lde_log > 0: the input holds the leading n >> lde_log words of every transform
    CosetTables cs;
    if (shift != 1u && c->plan.log_n > 0) {
        ShiftTable* st = nullptr;
        int rc = get_shift_table(c, shift, &st);
        if (rc) return rc;
        const int dir = inverse ? 1 : 0;
        cs.lo = st->d + st->lo_off[dir];
        cs.hi = st->d + st->hi_off[dir];
        cs.lowbits = st->lowbits;
        cs.s = st->s[dir];
    }
    switch (r.kind) {
    case ROUTE_COPY:
        if (d_in != d_out) HIPCHK(hipMemcpyAsync(d_out, d_in, batch * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        return 0;
    case ROUTE_ROW_SWEEP: {
        // n = 2^11 / 2^12 in launches of at least TOYNI_R2048_MIN_ROWS / TOYNI_R4096_MIN_ROWS transforms: one sweep, one / two waves per transform
        hipError_t err = hipSuccess;
        const bool ok = row2048_transform(c->plan, inverse ? c->d_inv : c->d_fwd, inverse, d_in, d_out, batch, [&](const PassArgs& a, uint64_t rows) {
            TOYNI_PASS_TIMER(c, s, inverse ? 1 : 0, 0);
            if (c->plan.log_n == 11) {
                uint64_t grid = (rows + Row2048::WAVES - 1) / Row2048::WAVES;
                if (grid > (uint64_t)c->num_cus) grid = (uint64_t)c->num_cus;     // one 1024-thread workgroup per CU (132 KiB of LDS + 15 KiB of twiddles)
                if (r.nt) hipLaunchKernelGGL((ntt_row2048_kernel<true>), dim3((unsigned)grid), dim3(Row2048::T), 0, s, a);
                else hipLaunchKernelGGL((ntt_row2048_kernel<false>), dim3((unsigned)grid), dim3(Row2048::T), 0, s, a);
            } else {
                const uint64_t ntiles = (rows + Row4096::ROWS - 1) / Row4096::ROWS;
                const uint64_t grid = ntiles < (uint64_t)c->num_cus ? ntiles : (uint64_t)c->num_cus;
                if (r.nt) hipLaunchKernelGGL((ntt_row4096_kernel<true>), dim3((unsigned)grid), dim3(Row4096::T), 0, s, a, (uint32_t)ntiles);
                else hipLaunchKernelGGL((ntt_row4096_kernel<false>), dim3((unsigned)grid), dim3(Row4096::T), 0, s, a, (uint32_t)ntiles);
            }
            err = hipGetLastError();
        }, cs);
        return ok ? (int)err : TOYNI_E_INVALID_SIZE;
    }
    case ROUTE_LDS_SWEEP: {
        // n = 2^13 .. 2^15: one sweep, the transform never leaves the workgroup's LDS (no intermediate buffer)
        hipError_t err = hipSuccess;
        const bool ok = lds_transform(c->plan, inverse ? c->d_inv : c->d_fwd, inverse, d_in, d_out, batch,
                                      [&](auto pass, const LdsArgs& g, uint64_t ntiles) {
                                          using L = decltype(pass);
                                          TOYNI_PASS_TIMER(c, s, inverse ? 1 : 0, 0);
                                          uint64_t grid = (uint64_t)c->num_cus * L::WG_PER_CU;  // as many workgroups as the LDS of a CU holds
                                          if (grid > ntiles) grid = ntiles;
                                          hipLaunchKernelGGL((ntt_lds_kernel<L>), dim3((unsigned)grid), dim3(L::T), 0, s, g, (uint32_t)ntiles);
                                          err = hipGetLastError();
                                      }, cs, launch_knobs().lds_rows);
        return ok ? (int)err : TOYNI_E_INVALID_SIZE;
    }
    case ROUTE_PASSES: break;
    }
    const NttPlan& plan = r.lat ? c->plan_lat : c->plan;
    if (c->plan.npasses > 1) {
        int rc = grow(c, s, (void**)&sc.d_work, &sc.work_words, r.chunk * n, sizeof(uint32_t));
        if (rc) return rc;
    }
    const uint32_t* tables = r.lat ? (inverse ? c->d_inv_lat : c->d_fwd_lat) : (inverse ? c->d_inv : c->d_fwd);
    for (size_t b0 = 0; b0 < batch; b0 += r.chunk) {
        const size_t nb = batch - b0 < r.chunk ? batch - b0 : r.chunk;
        int rc = lq ? run_passes<2>(c, plan, tables, inverse, d_in + b0 * n_in, sc.d_work, d_out + b0 * n, nb, s, cs, r.lde_log, r.nt)
                    : run_passes<0>(c, plan, tables, inverse, d_in + b0 * n_in, sc.d_work, d_out + b0 * n, nb, s, cs, r.lde_log, r.nt);
        if (rc) return rc;
    }
    return 0;
}

int get_shift_table(toyni_ntt_ctx* c, uint32_t shift, ShiftTable** out) {
    auto it = c->shifts.find(shift);
    if (it != c->shifts.end()) { *out = &it->second; return 0; }
    ShiftTable st;
    std::vector<uint32_t> blob;
    st.s[0] = shift;
    st.s[1] = bb_inv_host(shift);  // src/math/domain.rs:167
    for (int dir = 0; dir < 2; ++dir) append_two_level(blob, c->plan.log_n, st.s[dir], 1u, st.lo_off[dir], st.hi_off[dir], st.lowbits);
    HIPCHK(hipMalloc((void**)&st.d, blob.size() * sizeof(uint32_t)));
    hipError_t e = hipMemcpy(st.d, blob.data(), blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(st.d); return (int)e; }
    auto ins = c->shifts.emplace(shift, st);
    *out = &ins.first->second;
    return 0;
}

// Device-side staging of the context-free host-slice entry points (toyni_fri_fold_host, toyni_fri_fold_ext_host,
// toyni_merkle_commit_host): one grow-only set of buffers and one stream per device for the life of the process, so a call
// costs copies and kernels, not hipMalloc / hipFree pairs; the u64 -> u32 narrowing (and the zero-point check of the fold)
// runs on the device, not in a host loop.  One call at a time per device (mutex): these are blocking calls.
struct HostStage {
    std::mutex mu;
    hipStream_t stream = nullptr;
    void* buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[5] = {0, 0, 0, 0, 0};
    uint32_t* d_flag = nullptr;
};

int host_stage_acquire(HostStage** out, int* device) {
    static std::mutex reg_mu;
    static std::map<int, HostStage*> reg;  // never freed: process lifetime, like the reference's context cache (src/ntt.rs:128-141)
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return TOYNI_E_NO_DEVICE; }
    HIPCHK(hipGetDevice(device));
    std::lock_guard<std::mutex> lk(reg_mu);
    HostStage*& st = reg[*device];
    if (!st) {
        st = new HostStage();
        hipError_t e = hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMalloc((void**)&st->d_flag, sizeof(uint32_t));
        if (e != hipSuccess) { delete st; st = nullptr; reg.erase(*device); return (int)e; }
    }
    *out = st;
    return TOYNI_OK;
}

int host_stage_reserve(HostStage* st, int slot, size_t bytes) {
    if (st->cap[slot] >= bytes) return 0;
    HIPCHK(hipStreamSynchronize(st->stream));  // blocking entry points: the stream is idle here anyway
    if (st->buf[slot]) { HIPCHK(hipFree(st->buf[slot])); st->buf[slot] = nullptr; st->cap[slot] = 0; }
    HIPCHK(hipMalloc(&st->buf[slot], bytes));
    st->cap[slot] = bytes;
    return 0;
}

// the launch sequence of toyni_column_scan_device for up to SCAN_INLINE_COLUMNS columns
template <int OP>
void column_scan_launch(const ScanArgs& a, const ScanInit& in, unsigned cols, hipStream_t s) {
    if (a.single) {
        hipLaunchKernelGGL(column_scan_apply_kernel<OP>, dim3(1, cols), dim3(SCAN_THREADS), 0, s, a, in);
        return;
    }
    hipLaunchKernelGGL(column_scan_aggregate_kernel<OP>, dim3(a.ntiles, cols), dim3(SCAN_THREADS), 0, s, a);
    hipLaunchKernelGGL(column_scan_prefix_kernel<OP>, dim3(cols), dim3(SCAN_THREADS), 0, s, a, in);
    hipLaunchKernelGGL(column_scan_apply_kernel<OP>, dim3(a.ntiles, cols), dim3(SCAN_THREADS), 0, s, a, in);
}
// the launch sequence of toyni_column_scan_ext_device for up to EXT_ACCUM_INLINE_COLUMNS Ext columns
template <int OP>
void ext_accum_launch(const ExtAccumArgs& a, const ExtAccumSeeds& in, unsigned cols, hipStream_t s) {
    if (a.single) {
        hipLaunchKernelGGL(ext_accum_apply_kernel<OP>, dim3(1, cols), dim3(EXT_ACCUM_THREADS), 0, s, a, in);
        return;
    }
    hipLaunchKernelGGL(ext_accum_aggregate_kernel<OP>, dim3(a.ntiles, cols), dim3(EXT_ACCUM_THREADS), 0, s, a);
    hipLaunchKernelGGL(ext_accum_prefix_kernel<OP>, dim3(cols), dim3(EXT_ACCUM_THREADS), 0, s, a, in);
    hipLaunchKernelGGL(ext_accum_apply_kernel<OP>, dim3(a.ntiles, cols), dim3(EXT_ACCUM_THREADS), 0, s, a, in);
}
// the same for toyni_column_scan_ext_dc_device: the record instead of the shifts; step 2 is the kernel above
template <int OP>
void ext_accum_dc_launch(const ExtAccumArgs& a, const ExtAccumSeeds& in, const ExtAccumRecord* rec, unsigned cols, hipStream_t s) {
    if (a.single) {
        hipLaunchKernelGGL(extcol_apply_dc_kernel<OP>, dim3(1, cols), dim3(EXT_ACCUM_THREADS), 0, s, a, in, rec);
        return;
    }
    hipLaunchKernelGGL(extcol_aggregate_dc_kernel<OP>, dim3(a.ntiles, cols), dim3(EXT_ACCUM_THREADS), 0, s, a, rec);
    hipLaunchKernelGGL(ext_accum_prefix_kernel<OP>, dim3(cols), dim3(EXT_ACCUM_THREADS), 0, s, a, in);
    hipLaunchKernelGGL(extcol_apply_dc_kernel<OP>, dim3(a.ntiles, cols), dim3(EXT_ACCUM_THREADS), 0, s, a, in, rec);
}

bool is_pow2(size_t v) { return v && !(v & (v - 1)); }
int ilog2(size_t v) { int l = 0; while (((size_t)1 << l) < v) ++l; return l; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* toyni_error_string(int status) {
    switch (status) {
        case TOYNI_OK: return "success";
        case TOYNI_E_INVALID_SIZE: return "NTT size must be a power of two and at most 2^27";
        case TOYNI_E_NULL: return "null context or pointer";
        case TOYNI_E_ODD_LENGTH: return "Evaluations length must be even";
        case TOYNI_E_NO_DEVICE: return "no HIP device available";
        case TOYNI_E_ZERO_INVERSE: return "Cannot invert zero";
        case TOYNI_E_RANGE: return "argument out of range";
        case TOYNI_E_NO_RCCL: return "librccl could not be loaded (RCCL exchange requested)";
        case TOYNI_E_RCCL: return "an RCCL call failed";
        case TOYNI_E_NO_PEER_ACCESS: return "devices of the group have no direct peer access (TOYNI_ALLOW_STAGED_PEER=1 accepts host-staged copies)";
        case TOYNI_E_REENTRANT: return "entry point called on a context from inside that context's transcript callback";
        case TOYNI_E_SELF_CHECK: return "multi-device self-check failed: the exchange does not reproduce the single-device transform";
        default: return hipGetErrorString((hipError_t)status);
    }
}

int toyni_device_count(int* count) {
    if (!count) return TOYNI_E_NULL;
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); }
    return (int)e;
}

// the reference's extern block takes this name from libcudart (src/ntt.rs:102): same signature, same meaning, HIP devices
int cudaGetDeviceCount(int* count) { return toyni_device_count(count); }

int toyni_set_device(int device) { return (int)hipSetDevice(device); }

// newline-separated symbols of every kernel this process has launched through the library so far; returns the bytes needed
// (including the terminating 0) -- call with (nullptr, 0) for the size.  Diagnostics: tests/test_zz_kernel_coverage.py.
size_t toyni_launched_kernels(char* buf, size_t cap) {
    std::lock_guard<std::mutex> lk(launch_registry::mu());
    size_t need = 1;
    for (const auto& s : launch_registry::names()) need += s.size() + 1;
    if (buf && cap) {
        size_t at = 0;
        for (const auto& s : launch_registry::names()) {
            if (at + s.size() + 1 >= cap) break;
            std::memcpy(buf + at, s.data(), s.size());
            at += s.size();
            buf[at++] = '\n';
        }
        buf[at] = 0;
    }
    return need;
}

int toyni_ntt_ctx_create(uint32_t n, int device, toyni_ntt_ctx** out) {
    if (!out) return TOYNI_E_NULL;
    *out = nullptr;
    if (!is_pow2(n) || ilog2(n) > MAX_LOG_N) return TOYNI_E_INVALID_SIZE;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return TOYNI_E_NO_DEVICE; }
    if (device < 0) HIPCHK(hipGetDevice(&device));
    if (device >= count) return TOYNI_E_RANGE;
    DeviceGuard guard(device);
    toyni_ntt_ctx* c = new toyni_ntt_ctx();
    c->n = n;
    c->device = device;
    if (!build_plan(ilog2(n), c->plan)) { delete c; return TOYNI_E_INVALID_SIZE; }
    // read ONCE per process, never rewritten by later context creations (this used to be an unsynchronised write per create)
    static const size_t env_chunk = (size_t)env_u64("TOYNI_CHUNK_ELEMS", 0);
    c->chunk_elems = env_chunk;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
    }
    auto fail = [&](hipError_t e) { toyni_ntt_ctx_destroy(c); return (int)e; };
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&c->d_fwd, c->plan.fwd.size() * sizeof(uint32_t))) != hipSuccess) return fail(e);
    if ((e = hipMalloc((void**)&c->d_inv, c->plan.inv.size() * sizeof(uint32_t))) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(c->d_fwd, c->plan.fwd.data(), c->plan.fwd.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if ((e = hipMemcpy(c->d_inv, c->plan.inv.data(), c->plan.inv.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
    if (has_latency_plan(c->plan.log_n) && build_plan(c->plan.log_n, c->plan_lat, true)) {
        if ((e = hipMalloc((void**)&c->d_fwd_lat, c->plan_lat.fwd.size() * sizeof(uint32_t))) != hipSuccess) return fail(e);
        if ((e = hipMalloc((void**)&c->d_inv_lat, c->plan_lat.inv.size() * sizeof(uint32_t))) != hipSuccess) return fail(e);
        if ((e = hipMemcpy(c->d_fwd_lat, c->plan_lat.fwd.data(), c->plan_lat.fwd.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
        if ((e = hipMemcpy(c->d_inv_lat, c->plan_lat.inv.data(), c->plan_lat.inv.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) return fail(e);
        c->has_lat = true;
    }
    *out = c;
    return TOYNI_OK;
}

int toyni_ntt_ctx_destroy(toyni_ntt_ctx* c) {
    if (!c) return TOYNI_OK;
    {
        DeviceGuard guard(c->device);
        if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
        (void)hipFree(c->d_fwd);
        (void)hipFree(c->d_inv);
        (void)hipFree(c->d_fwd_lat);
        (void)hipFree(c->d_inv_lat);
        (void)hipDeviceSynchronize();  // user streams may still carry this context's kernels
        for (auto& kv : c->scratch) retire_scratch(c, kv.second, kv.first, false);
        for (size_t i = 0; i < c->retired.size(); ++i) { (void)hipFree(c->retired[i].ptr); c->retired[i].ptr = nullptr; }
        for (size_t i = 0; i < c->retired.size(); ++i) { drop_retired_event(c, i); c->retired[i].ev = nullptr; }
        c->retired.clear();
        for (auto& kv : c->shifts) (void)hipFree(kv.second.d);
        if (c->pipe.ready) {
            (void)hipStreamDestroy(c->pipe.in);
            (void)hipStreamDestroy(c->pipe.out);
            for (int k = 0; k < 2; ++k) {
                (void)hipEventDestroy(c->pipe.in_done[k]);
                (void)hipEventDestroy(c->pipe.comp_done[k]);
                (void)hipEventDestroy(c->pipe.out_done[k]);
                (void)hipFree(c->pipe.d_stage[k]);
                (void)hipFree(c->pipe.d_data[k]);
            }
        }
        (void)hipFree(c->d_ones);
        if (c->h_root) (void)hipHostFree(c->h_root);
#ifdef TOYNI_TOOLS
        for (auto& r : c->timing_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
#endif
    }
    delete c;
    return TOYNI_OK;
}

uint32_t toyni_ntt_ctx_n(const toyni_ntt_ctx* c) { return c ? c->n : 0; }
int toyni_ntt_ctx_device(const toyni_ntt_ctx* c) { return c ? c->device : -1; }
int toyni_ntt_ctx_passes(const toyni_ntt_ctx* c) { return c ? (c->plan.log_n == 0 ? 0 : c->plan.npasses) : -1; }
int toyni_ntt_ctx_passes_for(const toyni_ntt_ctx* c, size_t batch) {
    if (!c) return -1;
    return batch == 0 ? 0 : route_of(c, batch).launches;
}

#ifdef TOYNI_TOOLS  // include/toyni_hip_tools.h
int toyni_ntt_ctx_timing(toyni_ntt_ctx* c, int enable) {
    if (!c) return TOYNI_E_NULL;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    if (enable) {
        for (auto& r : c->timing_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
        c->timing_recs.clear();
    }
    c->timing = enable != 0;
    return TOYNI_OK;
}

int toyni_ntt_ctx_timing_read(toyni_ntt_ctx* c, float* ms_sum, uint32_t* launches) {
    if (!c || !ms_sum || !launches) return TOYNI_E_NULL;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    for (int i = 0; i < 2 * MAX_PASSES; ++i) { ms_sum[i] = 0.f; launches[i] = 0u; }
    hipError_t err = hipSuccess;
    for (auto& r : c->timing_recs) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(r.e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, r.e0, r.e1);
        if (e == hipSuccess && r.pass < MAX_PASSES) { ms_sum[r.dir * MAX_PASSES + r.pass] += ms; launches[r.dir * MAX_PASSES + r.pass] += 1u; }
        if (e != hipSuccess && err == hipSuccess) err = e;
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    c->timing_recs.clear();
    return (int)err;
}

#endif  // TOYNI_TOOLS

int toyni_ntt_ctx_set_chunk(toyni_ntt_ctx* c, size_t chunk_elems) {
    if (!c) return TOYNI_E_NULL;
    TOYNI_CTX_LOCK(c);
    c->chunk_elems = chunk_elems;
    return TOYNI_OK;
}

int toyni_ntt_device(toyni_ntt_ctx* c, const uint32_t* d_in, uint32_t* d_out, size_t batch, int inverse, void* stream) {
    if (!c || !d_in || !d_out) return TOYNI_E_NULL;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    return enqueue_transform(c, d_in, d_out, batch, inverse != 0, (hipStream_t)stream);
}

int toyni_coset_ntt_device(toyni_ntt_ctx* c, const uint32_t* d_in, uint32_t* d_out, size_t batch, uint32_t shift, int inverse, void* stream) {
    if (!c || !d_in || !d_out) return TOYNI_E_NULL;
    if (shift == 0 || shift >= BB_P) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    // forward: scale by shift^i then NTT (src/math/domain.rs:111,121); inverse: INTT then scale by shift^-i (:99-100);
    // shift == 1 is the plain transform (:155,166).  The scaling is fused into the first / last pass.
    return enqueue_transform(c, d_in, d_out, batch, inverse != 0, s, shift);
}

int toyni_lde_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, uint32_t* d_out, size_t batch, unsigned log_blowup, uint32_t shift, void* stream) {
    if (!c || !d_coeffs || !d_out) return TOYNI_E_NULL;
    if (shift == 0 || shift >= BB_P || (int)log_blowup > c->plan.log_n) return TOYNI_E_RANGE;
    if (log_blowup && d_coeffs == d_out) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    return enqueue_transform(c, d_coeffs, d_out, batch, false, (hipStream_t)stream, shift, (int)log_blowup);
}

// BabyBearDomain::fft(coeffs) as ONE call on host slices (src/math/domain.rs:107-123): `ncoeffs` <= n coefficients in, n
// evaluations on shift * <w_n> out.  Only the coefficients cross PCIe on the way in (the reference pads on the host and
// uploads all n elements, src/ntt.rs:233 via cuda/ntt_kernel.cu:254); the padding is implied on the device.
int toyni_lde_host(toyni_ntt_ctx* c, const uint64_t* h_coeffs, size_t ncoeffs, uint64_t* h_out, uint64_t shift) {
    if (!c || !h_out || (!h_coeffs && ncoeffs)) return TOYNI_E_NULL;
    shift %= BB_P;
    if (shift == 0 || ncoeffs > (size_t)c->n) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    const size_t n = c->n;
    if (ncoeffs == 0) { std::memset(h_out, 0, n * sizeof(uint64_t)); return TOYNI_OK; }  // the zero polynomial
    size_t compact = 1;
    while (compact < ncoeffs) compact <<= 1;
    const unsigned log_blowup = (unsigned)(c->plan.log_n - ilog2(compact));
    hipStream_t s = c->stream;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc;
    if ((rc = grow(c, s, (void**)&sc.d_stage64, &sc.stage64_elems, n, sizeof(uint64_t)))) return rc;
    if ((rc = grow(c, s, (void**)&sc.d_data32, &sc.data32_words, n, sizeof(uint32_t)))) return rc;
    if ((rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, compact, sizeof(uint32_t)))) return rc;
    HIPCHK(hipMemcpyAsync(sc.d_stage64, h_coeffs, ncoeffs * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(ncoeffs)), dim3(256), 0, s, sc.d_stage64, sc.d_lde32, ncoeffs);
    if (compact > ncoeffs) HIPCHK(hipMemsetAsync(sc.d_lde32 + ncoeffs, 0, (compact - ncoeffs) * sizeof(uint32_t), s));
    if ((rc = enqueue_transform(c, sc.d_lde32, sc.d_data32, 1, false, s, (uint32_t)shift, (int)log_blowup))) return rc;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(n)), dim3(256), 0, s, sc.d_data32, sc.d_stage64, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out, sc.d_stage64, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    reclaim_after_sync(c, s);
    return TOYNI_OK;
}

int toyni_ntt_device_u64(toyni_ntt_ctx* c, uint64_t* d_data, size_t batch, int inverse, void* stream) {
    if (!c || !d_data) return TOYNI_E_NULL;
    if ((uintptr_t)d_data & 7) return TOYNI_E_RANGE;   // u64 elements
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    const size_t total = batch * (size_t)c->n;
    if (!total) return TOYNI_OK;
    int rc = grow(c, s, (void**)&sc.d_data32, &sc.data32_words, total, sizeof(uint32_t));
    if (rc) return rc;
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(total)), dim3(256), 0, s, d_data, sc.d_data32, total);
    if ((rc = enqueue_transform(c, sc.d_data32, sc.d_data32, batch, inverse != 0, s))) return rc;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(total)), dim3(256), 0, s, sc.d_data32, d_data, total);
    return (int)hipGetLastError();
}

// bytes of one pipeline chunk of the pinned host-slice path (TOYNI_PIPE_CHUNK_BYTES; 0 = never pipeline)
static size_t pipe_chunk_bytes() { static const size_t v = (size_t)env_u64("TOYNI_PIPE_CHUNK_BYTES", (uint64_t)64 << 20); return v; }

static bool host_pointer_is_pinned(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }  // plain pageable memory: unknown to the runtime
    return attr.type == hipMemoryTypeHost;
}

// chunked, double-buffered, three streams; h_data is pinned.  Caller holds c->mu and the device guard.
static int host_transform_pipelined(toyni_ntt_ctx* c, uint64_t* h_data, size_t batch, uint32_t shift, int inverse, size_t chunk) {
    const size_t n = c->n;
    toyni_ntt_ctx::HostPipe& p = c->pipe;
    if (!p.ready) {
        HIPCHK(hipStreamCreateWithFlags(&p.in, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&p.out, hipStreamNonBlocking));
        for (int k = 0; k < 2; ++k) {
            HIPCHK(hipEventCreateWithFlags(&p.in_done[k], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&p.comp_done[k], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&p.out_done[k], hipEventDisableTiming));
        }
        p.ready = true;
    }
    if (p.cap_elems < chunk * n) {
        HIPCHK(hipStreamSynchronize(p.in));
        HIPCHK(hipStreamSynchronize(p.out));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 2; ++k) {
            if (p.d_stage[k]) HIPCHK(hipFree(p.d_stage[k]));
            if (p.d_data[k]) HIPCHK(hipFree(p.d_data[k]));
            p.d_stage[k] = nullptr;
            p.d_data[k] = nullptr;
        }
        p.cap_elems = 0;
        for (int k = 0; k < 2; ++k) {
            HIPCHK(hipMalloc((void**)&p.d_stage[k], chunk * n * sizeof(uint64_t)));
            HIPCHK(hipMalloc((void**)&p.d_data[k], chunk * n * sizeof(uint32_t)));
        }
        p.cap_elems = chunk * n;
    }
    hipStream_t comp = c->stream;
    // a failure part way must not return while copies to / from the caller's memory are still in flight
    struct DrainOnExit {
        hipStream_t a, b, c;
        ~DrainOnExit() { (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b); (void)hipStreamSynchronize(c); }
    } drain{p.in, comp, p.out};
    size_t k = 0;
    for (size_t b0 = 0; b0 < batch; b0 += chunk, ++k) {
        const size_t nb = batch - b0 < chunk ? batch - b0 : chunk, elems = nb * n;
        const int slot = (int)(k & 1);
        uint64_t* h = h_data + b0 * n;
        if (k >= 2) HIPCHK(hipStreamWaitEvent(p.in, p.out_done[slot], 0));   // the slot's previous download has left the staging buffer
        HIPCHK(hipMemcpyAsync(p.d_stage[slot], h, elems * sizeof(uint64_t), hipMemcpyHostToDevice, p.in));
        HIPCHK(hipEventRecord(p.in_done[slot], p.in));
        HIPCHK(hipStreamWaitEvent(comp, p.in_done[slot], 0));
        hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(elems)), dim3(256), 0, comp, (const uint64_t*)p.d_stage[slot], p.d_data[slot], elems);
        int rc = enqueue_transform(c, p.d_data[slot], p.d_data[slot], nb, inverse != 0, comp, shift);
        if (rc) return rc;
        hipLaunchKernelGGL(widen_kernel, dim3(grid_for(elems)), dim3(256), 0, comp, (const uint32_t*)p.d_data[slot], p.d_stage[slot], elems);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(p.comp_done[slot], comp));
        HIPCHK(hipStreamWaitEvent(p.out, p.comp_done[slot], 0));
        HIPCHK(hipMemcpyAsync(h, p.d_stage[slot], elems * sizeof(uint64_t), hipMemcpyDeviceToHost, p.out));
        HIPCHK(hipEventRecord(p.out_done[slot], p.out));
    }
    HIPCHK(hipStreamSynchronize(p.out));
    HIPCHK(hipStreamSynchronize(comp));
    reclaim_after_sync(c, comp);
    return TOYNI_OK;
}

static int host_transform(toyni_ntt_ctx* c, uint64_t* h_data, size_t batch, uint32_t shift, int inverse) {
    if (!c || !h_data) return TOYNI_E_NULL;
    if (shift == 0 || shift >= BB_P) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    const size_t total = batch * (size_t)c->n;
    if (!total) return TOYNI_OK;
    // pinned host memory and more than one chunk's worth of data: upload, kernels and download overlap
    if (pipe_chunk_bytes() && batch >= 2 && total * sizeof(uint64_t) >= 2 * pipe_chunk_bytes() && host_pointer_is_pinned(h_data)) {
        size_t chunk = pipe_chunk_bytes() / ((size_t)c->n * sizeof(uint64_t));
        if (chunk < 1) chunk = 1;
        if (chunk > (batch + 1) / 2) chunk = (batch + 1) / 2;
        return host_transform_pipelined(c, h_data, batch, shift, inverse, chunk);
    }
    hipStream_t s = c->stream;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc;
    if ((rc = grow(c, s, (void**)&sc.d_stage64, &sc.stage64_elems, total, sizeof(uint64_t)))) return rc;
    if ((rc = grow(c, s, (void**)&sc.d_data32, &sc.data32_words, total, sizeof(uint32_t)))) return rc;
    HIPCHK(hipMemcpyAsync(sc.d_stage64, h_data, total * sizeof(uint64_t), hipMemcpyHostToDevice, s));  // cuda/ntt_kernel.cu:254
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(total)), dim3(256), 0, s, sc.d_stage64, sc.d_data32, total);
    if ((rc = enqueue_transform(c, sc.d_data32, sc.d_data32, batch, inverse != 0, s, shift))) return rc;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(total)), dim3(256), 0, s, sc.d_data32, sc.d_stage64, total);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_data, sc.d_stage64, total * sizeof(uint64_t), hipMemcpyDeviceToHost, s));  // cuda/ntt_kernel.cu:267
    HIPCHK(hipStreamSynchronize(s));
    reclaim_after_sync(c, s);
    return TOYNI_OK;
}

int toyni_ntt_host(toyni_ntt_ctx* c, uint64_t* h_data, size_t batch, int inverse) { return host_transform(c, h_data, batch, 1u, inverse); }

// fft_ext / ifft_ext (src/math/domain.rs:129-151) on host slices: one call, one PCIe round trip.  The reference de-interleaves the
// four coordinates, transforms each and re-interleaves (:140-151); here the AoS vector goes through the interleaved passes as it is.
int toyni_ntt_ext_host(toyni_ntt_ctx* c, uint64_t* h_data, uint64_t shift, int inverse) {
    if (!c || !h_data) return TOYNI_E_NULL;
    shift %= BB_P;
    if (shift == 0) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    const size_t n = c->n, total = 4 * n;
    hipStream_t s = c->stream;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc;
    if ((rc = grow(c, s, (void**)&sc.d_stage64, &sc.stage64_elems, total, sizeof(uint64_t)))) return rc;
    if ((rc = grow(c, s, (void**)&sc.d_data32, &sc.data32_words, total, sizeof(uint32_t)))) return rc;
    HIPCHK(hipMemcpyAsync(sc.d_stage64, h_data, total * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(total)), dim3(256), 0, s, sc.d_stage64, sc.d_data32, total);
    if ((rc = enqueue_transform(c, sc.d_data32, sc.d_data32, 1, inverse != 0, s, (uint32_t)shift, 0, 2))) return rc;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(total)), dim3(256), 0, s, sc.d_data32, sc.d_stage64, total);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_data, sc.d_stage64, total * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    reclaim_after_sync(c, s);
    return TOYNI_OK;
}

// device-resident Ext transforms on AoS packed u32 (batch vectors of n elements x 4 coordinates): exactly the plan's passes, no
// de-interleave (round 4; rounds 2-3 split into four columns, ran a batch of 4 and joined: two extra sweeps)
int toyni_ntt_ext_batch_device(toyni_ntt_ctx* c, const uint32_t* d_in, uint32_t* d_out, size_t batch, uint32_t shift, int inverse, void* stream) {
    if (!c || !d_in || !d_out) return TOYNI_E_NULL;
    if (shift == 0 || shift >= BB_P) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    if (c->plan.log_n == 0) {   // n = 1: the identity on every coordinate
        if (d_in != d_out && batch) HIPCHK(hipMemcpyAsync(d_out, d_in, batch * 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return TOYNI_OK;
    }
    return enqueue_transform(c, d_in, d_out, batch, inverse != 0, (hipStream_t)stream, shift, 0, 2);
}

int toyni_ntt_ext_device(toyni_ntt_ctx* c, uint32_t* d_data, uint32_t shift, int inverse, void* stream) {
    return toyni_ntt_ext_batch_device(c, d_data, d_data, 1, shift, inverse, stream);
}

int toyni_coset_ntt_host(toyni_ntt_ctx* c, uint64_t* h_data, size_t batch, uint64_t shift, int inverse) {
    if (shift >= BB_P) shift %= BB_P;
    return host_transform(c, h_data, batch, (uint32_t)shift, inverse);
}

// fft_ext of short coefficient vectors (src/math/domain.rs:134-151 pads each coordinate column to the domain size): `batch` AoS vectors
// of n >> log_blowup Ext coefficients in, n Ext evaluations each out -- the interleaved low-degree extension, padding implied
int toyni_lde_ext_batch_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, uint32_t* d_out, size_t batch, unsigned log_blowup, uint32_t shift, void* stream) {
    if (!c || !d_coeffs || !d_out) return TOYNI_E_NULL;
    if (shift == 0 || shift >= BB_P || (int)log_blowup > c->plan.log_n || (log_blowup && d_coeffs == d_out)) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    if (c->plan.log_n == 0) {
        if (d_coeffs != d_out && batch) HIPCHK(hipMemcpyAsync(d_out, d_coeffs, batch * 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return TOYNI_OK;
    }
    return enqueue_transform(c, d_coeffs, d_out, batch, false, (hipStream_t)stream, shift, (int)log_blowup, 2);
}

int toyni_lde_ext_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, uint32_t* d_out, unsigned log_blowup, uint32_t shift, void* stream) {
    if (d_coeffs && d_coeffs == d_out) return TOYNI_E_RANGE;
    return toyni_lde_ext_batch_device(c, d_coeffs, d_out, 1, log_blowup, shift, stream);
}

int toyni_lde_ext_host(toyni_ntt_ctx* c, const uint64_t* h_coeffs, size_t ncoeffs, uint64_t* h_out, uint64_t shift) {
    if (!c || !h_out || (!h_coeffs && ncoeffs)) return TOYNI_E_NULL;
    shift %= BB_P;
    if (shift == 0 || ncoeffs > (size_t)c->n) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    const size_t n = c->n;
    if (ncoeffs == 0) { std::memset(h_out, 0, 4 * n * sizeof(uint64_t)); return TOYNI_OK; }
    size_t compact = 1;
    while (compact < ncoeffs) compact <<= 1;
    const unsigned log_blowup = (unsigned)(c->plan.log_n - ilog2(compact));
    hipStream_t s = c->stream;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc;
    if ((rc = grow(c, s, (void**)&sc.d_stage64, &sc.stage64_elems, 4 * n, sizeof(uint64_t)))) return rc;
    if ((rc = grow(c, s, (void**)&sc.d_data32, &sc.data32_words, 4 * n, sizeof(uint32_t)))) return rc;
    if ((rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, 4 * compact, sizeof(uint32_t)))) return rc;
    HIPCHK(hipMemcpyAsync(sc.d_stage64, h_coeffs, 4 * ncoeffs * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(4 * ncoeffs)), dim3(256), 0, s, sc.d_stage64, sc.d_lde32, 4 * ncoeffs);
    if (compact > ncoeffs) HIPCHK(hipMemsetAsync(sc.d_lde32 + 4 * ncoeffs, 0, 4 * (compact - ncoeffs) * sizeof(uint32_t), s));
    if (c->plan.log_n == 0) HIPCHK(hipMemcpyAsync(sc.d_data32, sc.d_lde32, 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    else if ((rc = enqueue_transform(c, sc.d_lde32, sc.d_data32, 1, false, s, (uint32_t)shift, (int)log_blowup, 2))) return rc;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(4 * n)), dim3(256), 0, s, sc.d_data32, sc.d_stage64, 4 * n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_out, sc.d_stage64, 4 * n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    reclaim_after_sync(c, s);
    return TOYNI_OK;
}

// ---- multi-GPU 4-step helper: the twiddle between the two local transform stages ----
int toyni_fourstep_twiddle_device(toyni_ntt_ctx* c, uint32_t* d_data, size_t rows, size_t row_len, size_t row0, int inverse, void* stream) {
    if (!c || !d_data) return TOYNI_E_NULL;
    if (!is_pow2(row_len) || (rows + row0) * row_len > (size_t)c->n || row_len > c->n) return TOYNI_E_RANGE;
    if (!rows) return TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    const uint32_t* t = inverse ? c->d_inv : c->d_fwd;
    const uint64_t total = (uint64_t)rows * row_len;
    hipLaunchKernelGGL(fourstep_twiddle_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, d_data, total, (uint32_t)ilog2(row_len),
                       (uint32_t)row0, t + c->plan.dom_lo_off, t + c->plan.dom_hi_off, c->plan.dom_lowbits);
    return (int)hipGetLastError();
}

// ---- one transform over several devices: the local stages either side of the caller's all-to-all ----
size_t toyni_ntt_ctx_first_pass_points(const toyni_ntt_ctx* c) {
    return (c && c->plan.npasses >= 2) ? (size_t)1 << c->plan.pass[0].log_m : 0;
}

// the same without a context (and without a device): the split rule of this process, for callers that lay out slabs before any
// context exists (toyni_amd/dist.py) -- one source for the rule instead of a re-derivation on the other side of the ABI
size_t toyni_first_pass_points(uint32_t n) {
    if (!is_pow2(n) || ilog2(n) > MAX_LOG_N) return 0;
    int npasses = 0, logm[MAX_PASSES] = {0, 0, 0};
    split_passes(launch_knobs(), ilog2(n), npasses, logm);
    return npasses >= 2 ? (size_t)1 << logm[0] : 0;
}

int toyni_ntt_slab_pass_device(toyni_ntt_ctx* c, uint32_t* d_slab, size_t cols_local, size_t col_base, int inverse, void* stream) {
    if (!c || !d_slab) return TOYNI_E_NULL;
    if (c->plan.npasses < 2) return TOYNI_E_INVALID_SIZE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    if (inverse && !c->d_ones) {
        const uint32_t lowbits = c->plan.pass[0].lowbits;
        const size_t words = (size_t)1 << (lowbits > c->plan.log_n - lowbits ? lowbits : c->plan.log_n - lowbits);
        std::vector<uint32_t> ones(words, to_mont_host(1u));
        HIPCHK(hipMalloc((void**)&c->d_ones, words * sizeof(uint32_t)));
        hipError_t e = hipMemcpy(c->d_ones, ones.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(c->d_ones); c->d_ones = nullptr; return (int)e; }
    }
    hipError_t err = hipSuccess;
    const bool ok = slab_pass(launch_knobs(), c->plan, inverse ? c->d_inv : c->d_fwd, inverse != 0, d_slab, cols_local, col_base, c->d_ones,
                              [&](auto pass, const PassArgs& a, uint64_t nblocks) {
                                  using P = decltype(pass);
                                  launch_pass<P>(persistent_grid<P>(c, nblocks), (hipStream_t)stream, a, (uint32_t)nblocks);
                                  err = hipGetLastError();
                              });
    if (!ok) return TOYNI_E_RANGE;
    return (int)err;
}

int toyni_ntt_slab_relayout_device(toyni_ntt_ctx* c, const uint32_t* d_in, uint32_t* d_out, size_t rows_local, size_t row0, size_t parts,
                                   int inverse, void* stream) {
    if (!c || !d_in || !d_out) return TOYNI_E_NULL;
    if (d_in == d_out || (((uintptr_t)d_in | (uintptr_t)d_out) & 15)) return TOYNI_E_RANGE;   // 16-byte accesses on both sides
    const size_t m1 = toyni_ntt_ctx_first_pass_points(c);
    if (!m1) return TOYNI_E_INVALID_SIZE;
    const size_t s1 = (size_t)c->n / m1;
    if (!is_pow2(rows_local) || !is_pow2(parts) || parts > s1 || s1 / parts < 32 || row0 + rows_local > m1) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    RelayoutArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.log_rows = (uint32_t)ilog2(rows_local);
    a.log_parts = (uint32_t)ilog2(parts);
    a.log_w = (uint32_t)ilog2(s1 / parts);
    a.inverse = inverse ? 1u : 0u;
    a.row0 = (uint32_t)row0;
    a.lo = c->d_inv + c->plan.dom_lo_off;
    a.hi = c->d_inv + c->plan.dom_hi_off;
    a.lowbits = c->plan.dom_lowbits;
    const uint64_t quads = ((uint64_t)rows_local * s1) / 4;
    hipLaunchKernelGGL(slab_relayout_kernel, dim3(grid_for(quads)), dim3(256), 0, (hipStream_t)stream, a, quads);
    return (int)hipGetLastError();
}

// Round 5: relayout + row transforms as ONE call, and -- where the dispatched pass shapes can address the pieces layout -- without
// the relayout sweep: the first pass of the forward row transforms reads [parts][rows][W] directly, the last pass of the inverse ones
// writes it (twiddled).  Three HBM sweeps per direction around the exchange instead of four.  Shapes that cannot (three-step latency
// shapes on small launches, fewer rows per piece than a thread's register stride, single-pass row transforms, one row) take the two
// separate steps: the results are identical either way.  *fused_out (optional): 1 = fused, 0 = the two-step form.
int toyni_ntt_slab_rows_device(toyni_ntt_ctx* big, toyni_ntt_ctx* row, uint32_t* d_in, uint32_t* d_out, size_t rows_local, size_t row0,
                               size_t parts, int inverse, int* fused_out, void* stream) {
    if (fused_out) *fused_out = 0;
    if (!big || !row || !d_in || !d_out) return TOYNI_E_NULL;
    if (d_in == d_out || (((uintptr_t)d_in | (uintptr_t)d_out) & 15)) return TOYNI_E_RANGE;   // (the relayout's 16-byte accesses)
    const size_t m1 = toyni_ntt_ctx_first_pass_points(big);
    if (!m1) return TOYNI_E_INVALID_SIZE;
    const size_t s1 = (size_t)big->n / m1;
    if (row->n != s1 || row->device != big->device) return TOYNI_E_RANGE;
    if (!is_pow2(rows_local) || !is_pow2(parts) || parts > s1 || s1 / parts < 32 || row0 + rows_local > m1) return TOYNI_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    bool fused = false;
    {
        TOYNI_CTX_LOCK(row);   // (big is only read: its tables are immutable after creation)
        DeviceGuard guard(row->device);
        // (a chunked context keeps its chunks, the sweeps have no pieces layout: the two-step form.  Rows are at most 2^20 points: never the latency plan)
        const Route r = route_of(row, rows_local);
        if (r.kind == ROUTE_PASSES && r.chunk >= rows_local && rows_local >= 2) {
            SlabIo sio;
            bool unsupported = false;
            sio.log_parts = (uint32_t)ilog2(parts);
            sio.tw_lo = big->d_inv + big->plan.dom_lo_off;
            sio.tw_hi = big->d_inv + big->plan.dom_hi_off;
            sio.tw_lowbits = big->plan.dom_lowbits;
            sio.row0 = (uint32_t)row0;
            sio.unsupported = &unsupported;
            sio.dry = true;
            const uint32_t* tables = inverse ? row->d_inv : row->d_fwd;
            auto nothing = [](auto, auto, const PassArgs&, uint64_t) {};
            bool ok = for_each_pass<0>(launch_knobs(), row->plan, tables, inverse != 0, d_in, nullptr, d_out, rows_local, nothing, CosetTables(), 0, r.nt, &sio);
            if (ok && !unsupported) {
                toyni_ntt_ctx::Scratch& sc = scratch_for(row, s);
                int rc = grow(row, s, (void**)&sc.d_work, &sc.work_words, rows_local * (size_t)row->n, sizeof(uint32_t));
                if (rc) return rc;
                sio.dry = false;
                rc = run_passes<0>(row, row->plan, tables, inverse != 0, d_in, sc.d_work, d_out, rows_local, s, CosetTables(), 0, r.nt, &sio);
                if (rc) return rc;
                if (unsupported) return TOYNI_E_INVALID_SIZE;   // cannot happen after the dry run said yes
                fused = true;
            }
        }
    }
    if (fused) {
        if (fused_out) *fused_out = 1;
        return TOYNI_OK;
    }
    // the two-step form (each call locks the context it uses)
    int rc;
    if (!inverse) {
        if ((rc = toyni_ntt_slab_relayout_device(big, d_in, d_out, rows_local, row0, parts, 0, stream))) return rc;
        return toyni_ntt_device(row, d_out, d_out, rows_local, 0, stream);
    }
    if ((rc = toyni_ntt_device(row, d_in, d_in, rows_local, 1, stream))) return rc;
    return toyni_ntt_slab_relayout_device(big, d_in, d_out, rows_local, row0, parts, 1, stream);
}

// ---- domain points (the xs of fri_fold, the evaluation points of the prover) ----
int toyni_domain_elements_device(toyni_ntt_ctx* c, uint32_t* d_out, size_t m, uint32_t shift, void* stream) {
    if (!c || !d_out) return TOYNI_E_NULL;
    if (m == 0) return TOYNI_OK;
    if (!is_pow2(m) || m > c->n || shift >= BB_P) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipLaunchKernelGGL(domain_elements_kernel, dim3(grid_for(m)), dim3(256), 0, (hipStream_t)stream, d_out, (uint64_t)m, shift,
                       sub_domain(c->plan, c->d_fwd, c->plan.log_n - ilog2(m)));
    return (int)hipGetLastError();
}

// ---- FRI fold ----
// input bytes from which a fold streams past the caches: the shaped-stream kernels with non-temporal accesses.  256 MiB = the Infinity
// Cache (TOYNI_FOLD_NT_MIN_BYTES; the transforms' gate, TOYNI_NT_MIN_BYTES, is 512 MiB).  Measured with tools/foldsweep.py, gate at 512 /
// 256 / 128 MiB: structured 2^26 layer (256 MiB in) 76.1 / 67.2 / 67.6 us, Ext 2^24 layer (256 MiB in) 77.5 / 68.2 / 68.7 us -- and at
// 128 MiB the layers that still fit the cache lose (structured 2^25: 33.7 -> 38.2 us, Ext 2^23: 31.2 -> 35.6).
static uint64_t fold_nt_min_bytes() { static const uint64_t v = env_u64("TOYNI_FOLD_NT_MIN_BYTES", (uint64_t)256 << 20); return v; }

static int fold_args(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, uint32_t beta, uint32_t x0, FoldArgs& f) {
    if (m % 2) return TOYNI_E_ODD_LENGTH;
    if (!is_pow2(m) || m > c->n) return TOYNI_E_RANGE;
    if (x0 == 0 || x0 >= BB_P || beta >= BB_P) return x0 == 0 ? TOYNI_E_ZERO_INVERSE : TOYNI_E_RANGE;
    f = FoldArgs{};
    f.evals = d_evals;
    f.out = d_out;
    f.dom = sub_domain(c->plan, c->d_inv, c->plan.log_n - ilog2(m));
    f.coef = to_mont_host(bb_mul_host(bb_mul_host(beta, BB_HALF), bb_inv_host(x0)));
    f.half = m / 2;
    f.step = to_mont_host(bb_inv_host(bb_root_of_unity_host((uint32_t)ilog2(m))));
    return TOYNI_OK;
}

static int enqueue_fold(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, uint32_t beta, uint32_t x0, hipStream_t s,
                        const uint8_t* d_salts = nullptr, uint8_t* d_leaves = nullptr) {
    if (m == 0) return TOYNI_OK;
    FoldArgs f;
    int rc = fold_args(c, d_evals, d_out, m, beta, x0, f);
    if (rc) return rc;
    const bool quads = !d_leaves && fold_quads(d_evals, d_out, f.half);
    const size_t work = quads ? f.half / 4 : f.half;
    const uint4* no_salts = nullptr;
    Digest* no_leaves = nullptr;
    if (d_leaves) {
        hipLaunchKernelGGL((fri_fold_kernel<false, true>), dim3(grid_for(work)), dim3(256), 0, s, f, reinterpret_cast<const uint4*>(d_salts),
                           reinterpret_cast<Digest*>(d_leaves));
    } else if (quads && m >= 64 && (uint64_t)m * sizeof(uint32_t) >= fold_nt_min_bytes()) {
        // layers beyond the Infinity Cache (>= 256 MiB of input): the shaped stream, 1024 threads x 2 load pairs in flight, non-temporal.
        // A cache-resident 2^24 layer is 5 % FASTER on the 256-thread kernel below (5.95 against 5.63 TB/s), so smaller layers keep it.
        // Measured on a 2^27 layer, alternating (profiles/r03_ab_fold_shape.txt): 5.45-5.47 TB/s for round 2's 256-thread kernel with
        // non-temporal accesses, 5.83 for its shape with fold_quad (256 x 4), 5.72 / 6.01-6.19 / 5.93 for 1024 x 4 / 1024 x 2 / 512 x 4
        // -- only the winner is instantiated (round 5: the A/B knob TOYNI_FOLD_SHAPE and the non-temporal twin of the 256-thread
        // kernel, which nothing but that knob could reach on a layer of more than 32 elements, are gone: ADVICE r4).  (Round 4: the gate was 2^26 elements with the non-temporal hint from
        // 512 MiB only, so a 2^26 layer streamed with plain accesses: 76 -> 67 us with the hint, tools/foldsweep.py.)
        const uint64_t quads = f.half / 4, chunk = 1024 * 2, cap = (uint64_t)c->num_cus * 8;
        uint64_t g = (quads + chunk - 1) / chunk;
        if (g > cap) g = cap;
        hipLaunchKernelGGL((fri_fold_stream_kernel<true, 1024, 2>), dim3((unsigned)g), dim3(1024), 0, s, f);
    } else {
        hipLaunchKernelGGL((fri_fold_kernel<false, false>), dim3(grid_for(work)), dim3(256), 0, s, f, no_salts, no_leaves);
    }
    return (int)hipGetLastError();
}

static int enqueue_merkle_upper(uint8_t* d_levels, size_t n, hipStream_t s, uint32_t* notify = nullptr, uint32_t seq = 0);

// One protocol round: fold (+ leaf hashes in the same sweep) and the node levels of the folded layer's tree (+ the root's
// notification).  Round 3 built the round of a small layer (<= 2^11 leaves) as ONE single-workgroup launch -- fold, leaves, every
// level, notify -- and measured it against these two launches: 41.8-118 us against 42.6-106 us per round for
// 16 ... 2048 leaves (profiles/r03_fri_rounds_fused_small.txt / _two_launch.txt): nothing, because a small round is not launch-bound
// but a chain of dependent SHA-256 compressions (3.3 us each on one wave: ~1 500 instructions at 5 cycles); not kept.
static int enqueue_fold_commit(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, uint32_t beta, uint32_t x0, hipStream_t s,
                               const uint8_t* d_salts, uint8_t* d_levels, uint32_t* notify, uint32_t seq) {
    int rc = enqueue_fold(c, d_evals, d_out, m, beta, x0, s, d_salts, d_levels);
    if (rc) return rc;
    return enqueue_merkle_upper(d_levels, m / 2, s, notify, seq);
}

int toyni_fri_fold_device(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, uint32_t beta, uint32_t x0, void* stream) {
    if (!c || !d_evals || !d_out) return TOYNI_E_NULL;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    return enqueue_fold(c, d_evals, d_out, m, beta, x0, (hipStream_t)stream);
}

int toyni_fri_fold_layers_device(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_layers, const uint32_t* betas, unsigned nfolds,
                                 uint32_t shift, void* stream) {
    if (!c || !d_evals || !d_layers || (!betas && nfolds)) return TOYNI_E_NULL;
    if (shift == 0 || shift >= BB_P) return TOYNI_E_ZERO_INVERSE;
    if (nfolds > (unsigned)c->plan.log_n) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t* cur = d_evals;
    uint32_t* dst = d_layers;
    size_t m = c->n;
    uint32_t x0 = shift;  // layer k points: (shift w^i)^(2^k) -- xs squared after every fold, src/fibonacci.rs:228-231
    for (unsigned k = 0; k < nfolds; ++k) {
        int rc = enqueue_fold(c, cur, dst, m, betas[k], x0, s);
        if (rc) return rc;
        cur = dst;
        dst += m / 2;
        m /= 2;
        x0 = bb_mul_host(x0, x0);
    }
    return TOYNI_OK;
}

int toyni_fri_fold_xs_device(const uint32_t* d_evals, const uint32_t* d_xs, uint32_t* d_out, size_t m, uint32_t beta, void* stream) {
    if (!d_evals || !d_xs || !d_out) return TOYNI_E_NULL;
    if (m % 2) return TOYNI_E_ODD_LENGTH;
    if (m == 0) return TOYNI_OK;
    if (beta >= BB_P) return TOYNI_E_RANGE;
    const uint64_t half = m / 2;
    const uint32_t beta_half = bb_mul_host(beta, BB_HALF);   // plain: batch_inverse_scaled folds it into the shared inverse
    // large layers of whole quads behind 16-byte aligned pointers: one inversion per 16 outputs.  Measured, alternating
    // (profiles/r03_ab_fold_xs16.txt): 2^24 layer 46.6 -> 26.7 us (2.9 -> 5.0 TB/s of its 8 B per input element), 2^27 418 -> 238 us;
    // a 2^20 layer LOSES (6.8 -> 9.0 us: 32 768 threads with a four times longer serial chain each), hence the size gate.
    // Round 4 (plain-form batch inversion, 41-product chain, coalesced quads): 2^24 23.8 us, 2^27 243 -> 186 us; with the shorter chain
    // the gate moved from 2^21 to 2^18 pairs (a 2^21-element layer 6.8 -> 4.4 us, 2^20 4.6 -> 4.0; below that every form sits on the
    // ~4 us launch floor).
    // TOYNI_FOLD_XS16=0: always the 4-per-inversion kernel (A/B).
    static const bool xs16 = [] { const char* e = std::getenv("TOYNI_FOLD_XS16"); return !(e && e[0] == '0'); }();
    if (xs16 && half >= ((uint64_t)1 << 18) && (half & 3) == 0 && !(((uintptr_t)d_evals | (uintptr_t)d_xs | (uintptr_t)d_out) & 15)) {
        constexpr int T = 256;
        const int grid = grid_for((half / 4 + 3) / 4, T);   // one thread per four quads
        if ((uint64_t)m * 4 >= fold_nt_min_bytes())
            hipLaunchKernelGGL((fri_fold_xs16_kernel<true, T>), dim3(grid), dim3(T), 0, (hipStream_t)stream, d_evals, d_xs, d_out, half, beta_half);
        else
            hipLaunchKernelGGL((fri_fold_xs16_kernel<false, T>), dim3(grid), dim3(T), 0, (hipStream_t)stream, d_evals, d_xs, d_out, half, beta_half);
    } else {
        hipLaunchKernelGGL(fri_fold_xs_kernel, dim3(grid_for((half + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_evals, d_xs, d_out, half, beta_half);
    }
    return (int)hipGetLastError();
}

static bool ext_beta_half(const uint32_t beta[4], ExtFactor* out) {
    uint32_t bh[4];
    for (int k = 0; k < 4; ++k) {
        if (beta[k] >= BB_P) return false;
        bh[k] = bb_mul_host(beta[k], BB_HALF);
    }
    *out = ext_factor_host(bh);
    return true;
}

int toyni_fri_fold_ext_device(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, const uint32_t beta[4], uint32_t x0, void* stream) {
    if (!c || !d_evals || !d_out || !beta) return TOYNI_E_NULL;
    if (m % 2) return TOYNI_E_ODD_LENGTH;
    if (m == 0) return TOYNI_OK;
    if (!is_pow2(m) || m > c->n) return TOYNI_E_RANGE;
    if (x0 == 0) return TOYNI_E_ZERO_INVERSE;
    if (((uintptr_t)d_evals | (uintptr_t)d_out) & 15) return TOYNI_E_RANGE;   // one 16-byte access per Ext element
    FoldExtArgs fa{};
    if (x0 >= BB_P || !ext_beta_half(beta, &fa.beta_half)) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    fa.base.evals = d_evals;
    fa.base.out = d_out;
    fa.base.dom = sub_domain(c->plan, c->d_inv, c->plan.log_n - ilog2(m));
    fa.base.coef = to_mont_host(bb_inv_host(x0));
    fa.base.half = m / 2;
    // streaming layers (>= TOYNI_FOLD_NT_MIN_BYTES = 256 MiB of input): the shaped stream, 5.0-5.2 -> 6.0 TB/s on a 2^25-element layer,
    // 5.2 -> 5.9 on a 2^24-element one (256 MiB in, 128 MiB out: past the Infinity Cache); a cache-resident 2^22-element layer is faster
    // on the 256-thread kernel (6.2 against 4.8 TB/s: profiles/r03_ab_fold_ext_shape.txt)
    if ((uint64_t)m * 16 >= fold_nt_min_bytes()) {
        const uint64_t chunk = 2 * 1024, cap = (uint64_t)c->num_cus * 8;
        uint64_t g = (fa.base.half + chunk - 1) / chunk;
        if (g > cap) g = cap;
        hipLaunchKernelGGL((fri_fold_ext_stream_kernel<true, 1024, 2>), dim3((unsigned)g), dim3(1024), 0, (hipStream_t)stream, fa);
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(fri_fold_ext_kernel, dim3(grid_for(fa.base.half)), dim3(256), 0, (hipStream_t)stream, fa);
    return (int)hipGetLastError();
}

int toyni_fri_fold_ext_xs_device(const uint32_t* d_evals, const uint32_t* d_xs, uint32_t* d_out, size_t m, const uint32_t beta[4], void* stream) {
    if (!d_evals || !d_xs || !d_out || !beta) return TOYNI_E_NULL;
    if (m % 2) return TOYNI_E_ODD_LENGTH;
    if (m == 0) return TOYNI_OK;
    ExtFactor f;
    if (!ext_beta_half(beta, &f) || (((uintptr_t)d_evals | (uintptr_t)d_out) & 15)) return TOYNI_E_RANGE;   // 16-byte Ext accesses
    const uint64_t half = m / 2;
    hipLaunchKernelGGL(fri_fold_ext_xs_kernel, dim3(grid_for((half + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(d_evals), d_xs, reinterpret_cast<uint4*>(d_out), half, f);
    return (int)hipGetLastError();
}

int toyni_fri_fold_ext_host(uint64_t* h_out, const uint64_t* h_evals, size_t len, const uint64_t* h_xs, const uint64_t beta[4]) {
    if (!h_out || !h_evals || !h_xs || !beta) return TOYNI_E_NULL;
    if (len % 2) return TOYNI_E_ODD_LENGTH;  // src/math/fri.rs:8
    if (len == 0) return TOYNI_OK;
    const size_t half = len / 2;
    uint32_t b32[4];
    for (int k = 0; k < 4; ++k) b32[k] = (uint32_t)(beta[k] % BB_P);
    HostStage* st = nullptr;
    int dev = 0, rc;
    if ((rc = host_stage_acquire(&st, &dev))) return rc;
    std::lock_guard<std::mutex> lk(st->mu);
    hipStream_t s = st->stream;
    // slots: 0 = evals u64 [4 len] (later the folded Ext values u32 [4 half]), 1 = xs u64 [half] , 2 = evals u32, 3 = xs u32, 4 = out u64 [4 half]
    if ((rc = host_stage_reserve(st, 0, 4 * len * sizeof(uint64_t)))) return rc;
    if ((rc = host_stage_reserve(st, 1, half * sizeof(uint64_t)))) return rc;
    if ((rc = host_stage_reserve(st, 2, 4 * len * sizeof(uint32_t)))) return rc;
    if ((rc = host_stage_reserve(st, 3, half * sizeof(uint32_t)))) return rc;
    if ((rc = host_stage_reserve(st, 4, 4 * half * sizeof(uint64_t)))) return rc;
    uint64_t* d_e64 = (uint64_t*)st->buf[0];
    uint64_t* d_x64 = (uint64_t*)st->buf[1];
    uint32_t* d_e32 = (uint32_t*)st->buf[2];
    uint32_t* d_x32 = (uint32_t*)st->buf[3];
    uint32_t* d_o32 = (uint32_t*)st->buf[0];
    uint64_t* d_o64 = (uint64_t*)st->buf[4];
    HIPCHK(hipMemsetAsync(st->d_flag, 0, sizeof(uint32_t), s));
    HIPCHK(hipMemcpyAsync(d_e64, h_evals, 4 * len * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_x64, h_xs, half * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(4 * len)), dim3(256), 0, s, (const uint64_t*)d_e64, d_e32, 4 * len);
    hipLaunchKernelGGL(narrow_nonzero_kernel, dim3(grid_for(half)), dim3(256), 0, s, (const uint64_t*)d_x64, d_x32, half, st->d_flag);
    if ((rc = toyni_fri_fold_ext_xs_device(d_e32, d_x32, d_o32, len, b32, s))) return rc;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(4 * half)), dim3(256), 0, s, (const uint32_t*)d_o32, d_o64, 4 * half);
    HIPCHK(hipGetLastError());
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, st->d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_out, d_o64, 4 * half * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return flag ? TOYNI_E_ZERO_INVERSE : TOYNI_OK;  // src/babybear.rs:112 (the reference panics before returning anything)
}

int toyni_fri_fold_host(uint64_t* h_out, const uint64_t* h_evals, size_t len, const uint64_t* h_xs, uint64_t beta) {
    if (!h_out || !h_evals || !h_xs) return TOYNI_E_NULL;
    if (len % 2) return TOYNI_E_ODD_LENGTH;  // src/math/fri.rs:28
    if (len == 0) return TOYNI_OK;
    const size_t half = len / 2;
    HostStage* st = nullptr;
    int dev = 0, rc;
    if ((rc = host_stage_acquire(&st, &dev))) return rc;
    std::lock_guard<std::mutex> lk(st->mu);
    hipStream_t s = st->stream;
    // slots: 0 = evals u64 [len] (later the folded layer u32 [half]), 1 = xs u64 [half] (later the output u64 [half]), 2 = evals u32, 3 = xs u32
    if ((rc = host_stage_reserve(st, 0, len * sizeof(uint64_t)))) return rc;
    if ((rc = host_stage_reserve(st, 1, half * sizeof(uint64_t)))) return rc;
    if ((rc = host_stage_reserve(st, 2, len * sizeof(uint32_t)))) return rc;
    if ((rc = host_stage_reserve(st, 3, half * sizeof(uint32_t)))) return rc;
    uint64_t* d_e64 = (uint64_t*)st->buf[0];
    uint64_t* d_x64 = (uint64_t*)st->buf[1];
    uint32_t* d_e32 = (uint32_t*)st->buf[2];
    uint32_t* d_x32 = (uint32_t*)st->buf[3];
    uint32_t* d_o32 = (uint32_t*)st->buf[0];
    HIPCHK(hipMemsetAsync(st->d_flag, 0, sizeof(uint32_t), s));
    HIPCHK(hipMemcpyAsync(d_e64, h_evals, len * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_x64, h_xs, half * sizeof(uint64_t), hipMemcpyHostToDevice, s));  // only xs[0 .. len/2) is read
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(len)), dim3(256), 0, s, (const uint64_t*)d_e64, d_e32, len);
    hipLaunchKernelGGL(narrow_nonzero_kernel, dim3(grid_for(half)), dim3(256), 0, s, (const uint64_t*)d_x64, d_x32, half, st->d_flag);
    if ((rc = toyni_fri_fold_xs_device(d_e32, d_x32, d_o32, len, (uint32_t)(beta % BB_P), s))) return rc;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(half)), dim3(256), 0, s, (const uint32_t*)d_o32, d_x64, half);
    HIPCHK(hipGetLastError());
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, st->d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_out, d_x64, half * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return flag ? TOYNI_E_ZERO_INVERSE : TOYNI_OK;  // src/babybear.rs:112
}

// ---- Merkle commitment ----
size_t toyni_merkle_total_digests(size_t n) {
    size_t total = 0;
    if (n == 0) return 0;
    for (;;) { total += n; if (n == 1) break; n = (n + 1) / 2; }
    return total;
}

// levels above the leaf hashes (already in d_levels[0 .. n))
int toyni_merkle_commit_device(const uint32_t* d_values, const uint8_t* d_salts, size_t n, uint8_t* d_levels, void* stream) {
    if (!d_values || !d_levels) return TOYNI_E_NULL;
    if (n == 0) return TOYNI_OK;
    if (((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15)) return TOYNI_E_RANGE;  // 16-byte accesses
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(merkle_leaf_kernel, dim3(grid_for(n)), dim3(256), 0, s, d_values, reinterpret_cast<const uint4*>(d_salts),
                       reinterpret_cast<Digest*>(d_levels), n);
    return enqueue_merkle_upper(d_levels, n, s);
}

static int enqueue_merkle_upper(uint8_t* d_levels, size_t n, hipStream_t s, uint32_t* notify, uint32_t seq) {
    Digest* cur = reinterpret_cast<Digest*>(d_levels);
    size_t m = n;
    // levels the chip cannot fill take the two-wave node hash (TOYNI_MERKLE_COOP_LOG = largest log2(nodes) that does; default 14,
    // -1 = never: A/B runs)
    static const int coop_log = env_int("TOYNI_MERKLE_COOP_LOG", 14);
    while (m > MERKLE_TAIL) {
        const size_t up = (m + 1) / 2;
        if (coop_log >= 0 && up <= ((size_t)1 << coop_log))
            hipLaunchKernelGGL(merkle_level_coop_kernel, dim3((unsigned)((up + 63) / 64)), dim3(128), 0, s, (const Digest*)cur, cur + m, m, up);
        else
            hipLaunchKernelGGL(merkle_level_kernel, dim3(grid_for(up)), dim3(256), 0, s, (const Digest*)cur, cur + m, m, up);
        cur += m;
        m = up;
    }
    if (m > 1) hipLaunchKernelGGL(merkle_tail_kernel, dim3(1), dim3(MERKLE_TAIL_T), 0, s, (const Digest*)cur, cur + m, (uint32_t)m, notify, seq);
    else if (notify) hipLaunchKernelGGL(merkle_notify_kernel, dim3(1), dim3(64), 0, s, (const Digest*)cur, notify, seq);  // a one-leaf tree: the leaf hash is the root
    return (int)hipGetLastError();
}

int toyni_merkle_commit_host(const uint64_t* h_values, const uint8_t* h_salts, size_t n, uint8_t* h_levels) {
    if (!h_values || !h_levels) return TOYNI_E_NULL;
    if (n == 0) return TOYNI_OK;
    HostStage* st = nullptr;
    int dev = 0, rc;
    if ((rc = host_stage_acquire(&st, &dev))) return rc;
    std::lock_guard<std::mutex> lk(st->mu);
    hipStream_t s = st->stream;
    const size_t total = toyni_merkle_total_digests(n);
    // slots: 0 = values u64, 1 = salts, 2 = values u32, 4 = all levels
    if ((rc = host_stage_reserve(st, 0, n * sizeof(uint64_t)))) return rc;
    if (h_salts && (rc = host_stage_reserve(st, 1, n * 16))) return rc;
    if ((rc = host_stage_reserve(st, 2, n * sizeof(uint32_t)))) return rc;
    if ((rc = host_stage_reserve(st, 4, total * 32))) return rc;
    HIPCHK(hipMemcpyAsync(st->buf[0], h_values, n * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (h_salts) HIPCHK(hipMemcpyAsync(st->buf[1], h_salts, n * 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const uint64_t*)st->buf[0], (uint32_t*)st->buf[2], n);
    if ((rc = toyni_merkle_commit_device((const uint32_t*)st->buf[2], h_salts ? (const uint8_t*)st->buf[1] : nullptr, n, (uint8_t*)st->buf[4], s))) return rc;
    HIPCHK(hipMemcpyAsync(h_levels, st->buf[4], total * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TOYNI_OK;
}

// ---- row leaves of a multi-column matrix (include/toyni_hip.h 3d) ----
constexpr size_t MERKLE_ROWS_MAX_WIDTH = 65536;
size_t toyni_merkle_row_leaf_bytes(size_t width, int salted) { return (salted ? 16u : 0u) + 8u * width; }

static int rows_args_check(size_t n, size_t width, int layout, size_t col_stride) {
    if (width == 0 || width > MERKLE_ROWS_MAX_WIDTH) return TOYNI_E_RANGE;
    if (layout != TOYNI_ROWS_COLUMN_MAJOR && layout != TOYNI_ROWS_ROW_MAJOR) return TOYNI_E_RANGE;
    if (layout == TOYNI_ROWS_COLUMN_MAJOR && col_stride < n) return TOYNI_E_RANGE;
    return TOYNI_OK;
}

int toyni_merkle_commit_rows_device(const uint32_t* d_values, size_t n, size_t width, int layout, size_t col_stride, const uint8_t* d_salts,
                                    uint8_t* d_levels, void* stream) {
    if (!d_values || !d_levels) return TOYNI_E_NULL;
    if (int rc = rows_args_check(n, width, layout, col_stride)) return rc;
    if (((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15) || ((uintptr_t)d_values & 3)) return TOYNI_E_RANGE;
    if (n == 0) return TOYNI_OK;
    hipStream_t s = (hipStream_t)stream;
    const uint4* salts = reinterpret_cast<const uint4*>(d_salts);
    Digest* out = reinterpret_cast<Digest*>(d_levels);
    const uint32_t w = (uint32_t)width;
    const bool vec = layout == TOYNI_ROWS_ROW_MAJOR && width % 4 == 0 && !((uintptr_t)d_values & 15);
    const dim3 grid(grid_for(n)), block(256);
    if (layout == TOYNI_ROWS_COLUMN_MAJOR) {
        if (salts) hipLaunchKernelGGL((merkle_rows_leaf_kernel<TOYNI_ROWS_COLUMN_MAJOR, true>), grid, block, 0, s, d_values, salts, out, n, w, col_stride, vec);
        else hipLaunchKernelGGL((merkle_rows_leaf_kernel<TOYNI_ROWS_COLUMN_MAJOR, false>), grid, block, 0, s, d_values, salts, out, n, w, col_stride, vec);
    } else {
        if (salts) hipLaunchKernelGGL((merkle_rows_leaf_kernel<TOYNI_ROWS_ROW_MAJOR, true>), grid, block, 0, s, d_values, salts, out, n, w, col_stride, vec);
        else hipLaunchKernelGGL((merkle_rows_leaf_kernel<TOYNI_ROWS_ROW_MAJOR, false>), grid, block, 0, s, d_values, salts, out, n, w, col_stride, vec);
    }
    return enqueue_merkle_upper(d_levels, n, s);
}

int toyni_merkle_commit_rows_host(const uint64_t* h_values, size_t n, size_t width, const uint8_t* h_salts, uint8_t* h_levels) {
    if (!h_values || !h_levels) return TOYNI_E_NULL;
    if (int rc = rows_args_check(n, width, TOYNI_ROWS_ROW_MAJOR, 0)) return rc;
    if (n == 0) return TOYNI_OK;
    HostStage* st = nullptr;
    int dev = 0, rc;
    if ((rc = host_stage_acquire(&st, &dev))) return rc;
    std::lock_guard<std::mutex> lk(st->mu);
    hipStream_t s = st->stream;
    const size_t total = toyni_merkle_total_digests(n), elems = n * width;
    // slots: 0 = values u64, 1 = salts, 2 = values u32, 4 = all levels
    if ((rc = host_stage_reserve(st, 0, elems * sizeof(uint64_t)))) return rc;
    if (h_salts && (rc = host_stage_reserve(st, 1, n * 16))) return rc;
    if ((rc = host_stage_reserve(st, 2, elems * sizeof(uint32_t)))) return rc;
    if ((rc = host_stage_reserve(st, 4, total * 32))) return rc;
    HIPCHK(hipMemcpyAsync(st->buf[0], h_values, elems * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (h_salts) HIPCHK(hipMemcpyAsync(st->buf[1], h_salts, n * 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(elems)), dim3(256), 0, s, (const uint64_t*)st->buf[0], (uint32_t*)st->buf[2], elems);
    if ((rc = toyni_merkle_commit_rows_device((const uint32_t*)st->buf[2], n, width, TOYNI_ROWS_ROW_MAJOR, 0, h_salts ? (const uint8_t*)st->buf[1] : nullptr,
                                              (uint8_t*)st->buf[4], s))) return rc;
    HIPCHK(hipMemcpyAsync(h_levels, st->buf[4], total * 32, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return TOYNI_OK;
}

size_t toyni_merkle_open_rows_record_bytes(size_t n, size_t width) {
    if (n == 0) return 0;
    const size_t d = merkle_depth(n);
    return d * 32u + 16u + 8u * width + ((d + 7u) & ~(size_t)7u);
}

int toyni_merkle_open_rows_device(const uint8_t* d_levels, size_t n, const uint32_t* d_values, size_t width, int layout, size_t col_stride,
                                  const uint8_t* d_salts, const uint32_t* d_indices, size_t nidx, uint8_t* d_out, void* stream) {
    if (!d_levels || !d_values || !d_indices || !d_out) return TOYNI_E_NULL;
    if (int rc = rows_args_check(n, width, layout, col_stride)) return rc;
    if (n > 0xFFFFFFFFull || nidx > 0xFFFFFFFFull || ((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15) || ((uintptr_t)d_out & 7) ||
        ((uintptr_t)d_values & 3) || ((uintptr_t)d_indices & 3)) return TOYNI_E_RANGE;
    if (n == 0 || nidx == 0) return TOYNI_OK;
    const uint64_t work = (uint64_t)nidx * (merkle_depth(n) + 1 + width);
    const OpenRows g{reinterpret_cast<const Digest*>(d_levels), (uint64_t)n, d_values, (uint32_t)width, layout, (uint64_t)col_stride,
                     reinterpret_cast<const uint4*>(d_salts), d_indices, (uint32_t)nidx, d_out};
    hipLaunchKernelGGL(merkle_open_rows_kernel, dim3(grid_for(work)), dim3(256), 0, (hipStream_t)stream, g);
    return (int)hipGetLastError();
}

// ---- fold + commit, pointwise prover steps (include/toyni_hip.h 3c) ----
// src/fibonacci.rs:222-245, one protocol round on the device: fold layer k with beta_k, and commit the folded layer (leaf
// hashes in the same sweep, then the node levels).  The NEXT beta depends on this commitment's root (the transcript absorbs it
// before the next squeeze, :242-243), so rounds cannot be fused further: the caller reads the root (last 32 bytes of the levels),
// derives beta and calls again.
int toyni_fri_fold_commit_device(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, uint32_t beta, uint32_t x0,
                                 const uint8_t* d_salts, uint8_t* d_levels, void* stream) {
    if (!c || !d_evals || !d_out || !d_levels) return TOYNI_E_NULL;
    if (((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15)) return TOYNI_E_RANGE;
    if (m < 2) return m % 2 ? TOYNI_E_ODD_LENGTH : TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    return enqueue_fold_commit(c, d_evals, d_out, m, beta, x0, s, d_salts, d_levels, nullptr, 0);
}

// spin on a word of pinned host memory until the device has stored `want` there (false after `seconds`)
static bool poll_until(volatile uint32_t* flag, uint32_t want, double seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; ++spins) {
        if (*flag == want) return true;
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
        if ((spins & 1023u) == 1023u && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
    }
}

// The fold loop of the commit phase, src/fibonacci.rs:222-245, with the transcript on the caller's side of a callback.  One loop for
// both element types: `words` = u32 words per layer element (1 base field, 4 Ext), Beta = uint32_t or ExtBeta,
//   challenge(round, prev_root32 or nullptr, Beta* or nullptr) -> int      the caller's callback
//   enqueue_round(cur, out, m, beta, x, salts, levels, notify, seq) -> int  one fold + commit; refuses a beta outside the field
// The arguments have been checked by the entry point.
extern "C++" template <class Beta, class Challenge, class Round>
static int commit_phase_loop(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size, size_t words,
                             const uint8_t* d_salts, uint32_t* d_layers, uint8_t* d_levels, uint8_t* h_roots, unsigned* rounds_out,
                             hipStream_t s, Challenge&& challenge, Round&& enqueue_round) {
    if (rounds_out) *rounds_out = 0;
    if (m0 <= final_size) return TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    if (!c->h_root) {
        // 32-byte root, then the sequence word, in pinned host memory that the device writes mid-stream with a system-scope release
        // store: that needs fine-grained (coherent) memory, so it is asked for explicitly rather than left to HIP_HOST_COHERENT.
        // Both pointers are published together or not at all (a half set-up pair made every later call poll for 2 s).
        uint8_t* h = nullptr;
        uint32_t* d = nullptr;
        HIPCHK(hipHostMalloc((void**)&h, 64, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(h, 0, 64);
        const hipError_t e = hipHostGetDevicePointer((void**)&d, h, 0);
        if (e != hipSuccess || !d) { (void)hipHostFree(h); return e != hipSuccess ? (int)e : TOYNI_E_NULL; }
        c->h_root = h;
        c->d_root_notify = d;
    }
    volatile uint32_t* flag = reinterpret_cast<volatile uint32_t*>(c->h_root) + 8;
    // the call is blocking on EVERY path: a callback that fails, or an error half way, must not leave kernels running on buffers the
    // caller is about to release
    struct DrainOnExit { hipStream_t st; ~DrainOnExit() { (void)hipStreamSynchronize(st); } } drain{s};
    const uint32_t* cur = d_layer0;
    uint32_t* out = d_layers;
    uint8_t* levels = d_levels;
    const uint8_t* salts = d_salts;
    uint32_t x = x0;
    unsigned round = 0;
    bool have_root = false;
    for (size_t m = m0; m > final_size; m >>= 1, ++round) {
        Beta beta{};
        int rc;
        {
            CallbackScope scope(c);
            rc = challenge(round, have_root ? c->h_root : nullptr, &beta);
        }
        if (rc) return rc;
        const size_t half = m >> 1;
        const bool last = half == final_size;
        const size_t digests = toyni_merkle_total_digests(half);
        const uint32_t seq = ++c->root_seq ? c->root_seq : ++c->root_seq;   // never 0
        if ((rc = enqueue_round(cur, out, m, beta, x, last ? nullptr : salts, levels, c->d_root_notify, seq))) return rc;
        // The tree's last kernel writes the root and then `seq` into pinned host memory; everything enqueued before it on `s` has
        // completed by then (stream order).  Polling costs ~2 us where a 32-byte copy plus a stream synchronisation costs ~16.
        if (!poll_until(flag, seq, 2.0)) {
            HIPCHK(hipStreamSynchronize(s));   // never observed; kept so that a lost notification degrades to the slow path
            if (*flag != seq) HIPCHK(hipMemcpy(c->h_root, levels + (digests - 1) * 32, 32, hipMemcpyDeviceToHost));
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        have_root = true;
        if (h_roots) std::memcpy(h_roots + (size_t)round * 32, c->h_root, 32);
        cur = out;
        out += half * words;
        levels += digests * 32;
        if (salts && !last) salts += half * 16;
        x = (uint32_t)((uint64_t)x * x % BB_P);   // the squared domain of the next layer, :228-231
    }
    if (rounds_out) *rounds_out = round;
    HIPCHK(hipStreamSynchronize(s));   // the call is blocking: the layers and trees are complete when it returns
    reclaim_after_sync(c, s);
    CallbackScope scope(c);
    return challenge(round, c->h_root, static_cast<Beta*>(nullptr));   // the transcript absorbs the last commitment too, :242-243
}

int toyni_fri_commit_phase_device(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                  const uint8_t* d_salts, toyni_fri_challenge_fn challenge, void* user, uint32_t* d_layers,
                                  uint8_t* d_levels, uint8_t* h_roots, unsigned* rounds_out, void* stream) {
    if (!c || !d_layer0 || !challenge || !d_layers || !d_levels) return TOYNI_E_NULL;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1 || m0 > c->n) return TOYNI_E_INVALID_SIZE;
    if (x0 == 0 || x0 >= BB_P) return TOYNI_E_RANGE;
    if (((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15)) return TOYNI_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    return commit_phase_loop<uint32_t>(
        c, d_layer0, m0, x0, final_size, 1, d_salts, d_layers, d_levels, h_roots, rounds_out, s,
        [&](unsigned round, const uint8_t* root, uint32_t* beta) { return challenge(user, round, root, beta); },
        [&](const uint32_t* cur, uint32_t* out, size_t m, uint32_t beta, uint32_t x, const uint8_t* salts, uint8_t* levels, uint32_t* notify,
            uint32_t seq) {
            if (beta >= BB_P) return (int)TOYNI_E_RANGE;
            return enqueue_fold_commit(c, cur, out, m, beta, x, s, salts, levels, notify, seq);
        });
}

// ---- the same round and the same phase over Ext-valued layers (include/toyni_hip.h 3j) ----
// fold (+ the width-4 row leaves in the same sweep), then the node levels and the root's notification through enqueue_merkle_upper.
// Arguments checked by the caller: m >= 2 a power of two <= n, x0 in [1, p), 16-byte aligned pointers.
static int enqueue_fold_commit_ext(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, const ExtFactor& beta_half, uint32_t x0,
                                   hipStream_t s, const uint8_t* d_salts, uint8_t* d_levels, uint32_t* notify, uint32_t seq) {
    FoldExtArgs fa{};
    fa.beta_half = beta_half;
    fa.base.evals = d_evals;
    fa.base.out = d_out;
    fa.base.dom = sub_domain(c->plan, c->d_inv, c->plan.log_n - ilog2(m));
    fa.base.coef = to_mont_host(bb_inv_host(x0));
    fa.base.half = m / 2;
    const dim3 grid(grid_for(fa.base.half)), block(256);
    Digest* leaves = reinterpret_cast<Digest*>(d_levels);
    if (d_salts) hipLaunchKernelGGL((fri_fold_ext_commit_kernel<true>), grid, block, 0, s, fa, reinterpret_cast<const uint4*>(d_salts), leaves);
    else hipLaunchKernelGGL((fri_fold_ext_commit_kernel<false>), grid, block, 0, s, fa, static_cast<const uint4*>(nullptr), leaves);
    return enqueue_merkle_upper(d_levels, m / 2, s, notify, seq);
}

int toyni_fri_fold_commit_ext_device(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, const uint32_t beta[4], uint32_t x0,
                                     const uint8_t* d_salts, uint8_t* d_levels, void* stream) {
    // every refusal that the arguments alone decide comes before the context is read
    if (!c || !d_evals || !d_out || !beta || !d_levels) return TOYNI_E_NULL;
    if (m % 2) return TOYNI_E_ODD_LENGTH;
    if (!is_pow2(m) && m) return TOYNI_E_RANGE;
    if (x0 == 0) return TOYNI_E_ZERO_INVERSE;
    if (((uintptr_t)d_evals | (uintptr_t)d_out | (uintptr_t)d_levels | (uintptr_t)d_salts) & 15) return TOYNI_E_RANGE;   // 16-byte accesses
    ExtFactor beta_half;
    if (x0 >= BB_P || !ext_beta_half(beta, &beta_half)) return TOYNI_E_RANGE;
    if (m == 0) return TOYNI_OK;
    if (m > c->n) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    return enqueue_fold_commit_ext(c, d_evals, d_out, m, beta_half, x0, (hipStream_t)stream, d_salts, d_levels, nullptr, 0);
}

struct ExtBeta { uint32_t v[4]; };
int toyni_fri_commit_phase_ext_device(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                      const uint8_t* d_salts, toyni_fri_ext_challenge_fn challenge, void* user, uint32_t* d_layers,
                                      uint8_t* d_levels, uint8_t* h_roots, unsigned* rounds_out, void* stream) {
    if (!c || !d_layer0 || !challenge || !d_layers || !d_levels) return TOYNI_E_NULL;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1) return TOYNI_E_INVALID_SIZE;
    if (x0 == 0) return TOYNI_E_ZERO_INVERSE;
    if (x0 >= BB_P) return TOYNI_E_RANGE;
    if (((uintptr_t)d_layer0 | (uintptr_t)d_layers | (uintptr_t)d_levels | (uintptr_t)d_salts) & 15) return TOYNI_E_RANGE;
    if (m0 > c->n) return TOYNI_E_INVALID_SIZE;
    hipStream_t s = (hipStream_t)stream;
    return commit_phase_loop<ExtBeta>(
        c, d_layer0, m0, x0, final_size, 4, d_salts, d_layers, d_levels, h_roots, rounds_out, s,
        [&](unsigned round, const uint8_t* root, ExtBeta* beta) { return challenge(user, round, root, beta ? beta->v : nullptr); },
        [&](const uint32_t* cur, uint32_t* out, size_t m, const ExtBeta& beta, uint32_t x, const uint8_t* salts, uint8_t* levels,
            uint32_t* notify, uint32_t seq) {
            ExtFactor beta_half;
            if (!ext_beta_half(beta.v, &beta_half)) return (int)TOYNI_E_RANGE;
            return enqueue_fold_commit_ext(c, cur, out, m, beta_half, x, s, salts, levels, notify, seq);
        });
}

// ---- the transcript in device memory and the commit phases on it (include/toyni_hip.h 3l) ----
static TranscriptState* transcript_of(toyni_transcript* d_tr) { return reinterpret_cast<TranscriptState*>(d_tr); }

int toyni_transcript_absorb_device(toyni_transcript* d_tr, const uint8_t* d_bytes, size_t len, void* stream) {
    if (!d_tr || (!d_bytes && len)) return TOYNI_E_NULL;
    if (((uintptr_t)d_tr & 15) || len > TOYNI_TRANSCRIPT_CAPACITY) return TOYNI_E_RANGE;
    if (len == 0) return TOYNI_OK;
    hipLaunchKernelGGL(transcript_absorb_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr), d_bytes, (uint32_t)len);
    return (int)hipGetLastError();
}

int toyni_transcript_squeeze_device(toyni_transcript* d_tr, uint32_t* d_out, size_t count, void* stream) {
    if (!d_tr || !d_out) return TOYNI_E_NULL;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_out & 3) || count > 65536) return TOYNI_E_RANGE;
    if (count == 0) return TOYNI_OK;
    hipLaunchKernelGGL(transcript_squeeze_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr), d_out, (uint32_t)count);
    return (int)hipGetLastError();
}

int toyni_transcript_squeeze_indices_device(toyni_transcript* d_tr, size_t count, uint32_t max, uint32_t* d_out, void* stream) {
    if (!d_tr || !d_out) return TOYNI_E_NULL;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_out & 3)) return TOYNI_E_RANGE;
    if (count == 0 || count > TRANSCRIPT_MAX_INDICES || max == 0 || count > max) return TOYNI_E_RANGE;
    hipLaunchKernelGGL(transcript_squeeze_indices_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr), (uint32_t)count, max,
                       d_out);
    return (int)hipGetLastError();
}

// ---- the proof-of-work nonce (include/toyni_hip.h 3n): arm, search, finish on the word d_nonce ----
int toyni_transcript_grind_device(toyni_transcript* d_tr, unsigned bits, uint64_t start, unsigned log_tries, uint64_t* d_nonce, void* stream) {
    if (!d_tr || !d_nonce) return TOYNI_E_NULL;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_nonce & 7)) return TOYNI_E_RANGE;
    if (bits > TOYNI_POW_MAX_BITS || log_tries > TOYNI_POW_MAX_LOG_TRIES) return TOYNI_E_RANGE;
    const uint64_t tries = (uint64_t)1 << log_tries;
    if (start > ~(uint64_t)0 - (tries - 1u)) return TOYNI_E_RANGE;   // start + 2^log_tries would pass 2^64
    const hipStream_t s = (hipStream_t)stream;
    TranscriptState* tr = transcript_of(d_tr);
    hipLaunchKernelGGL(pow_arm_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, tr, d_nonce);
    hipLaunchKernelGGL(pow_search_kernel, dim3(pow_grid_blocks(bits, log_tries)), dim3(POW_T), 0, s, static_cast<const TranscriptState*>(tr), (uint32_t)bits,
                       start, tries, d_nonce);
    hipLaunchKernelGGL(pow_finish_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, tr, d_nonce, (uint32_t)bits,
                       start + (tries - 1u) == ~(uint64_t)0 ? 1u : 0u);
    return (int)hipGetLastError();
}

int toyni_pow_check_host(const uint8_t* state, size_t len, uint64_t nonce, unsigned bits, int* accepted) {
    if (!accepted || (!state && len)) return TOYNI_E_NULL;
    if (bits > TOYNI_POW_MAX_BITS) return TOYNI_E_RANGE;
    *accepted = pow_check_bytes(state, (uint64_t)len, nonce, (uint32_t)bits) ? 1 : 0;
    return TOYNI_OK;
}

int toyni_fri_query_positions_device(const uint32_t* d_indices, size_t count, size_t m0, size_t final_size, uint32_t* d_out, void* stream) {
    if (!d_indices || !d_out) return TOYNI_E_NULL;
    if (((uintptr_t)d_indices & 3) || ((uintptr_t)d_out & 3)) return TOYNI_E_RANGE;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1 || (uint64_t)m0 > ((uint64_t)1 << 32) || count > 65536) return TOYNI_E_RANGE;
    if (count == 0 || m0 <= final_size) return TOYNI_OK;
    const uint64_t total = (uint64_t)(ilog2(m0) - ilog2(final_size)) * 2u * count;
    hipLaunchKernelGGL(fri_query_positions_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, d_indices, (uint32_t)count, (uint64_t)m0,
                       total, d_out);
    return (int)hipGetLastError();
}

// The loop of both transcript phases (arguments checked by the entry points; m0 > final_size).  `words` = u32 words per layer
// element.  Round k: its fold reads record k of the stream's buffer -- written by the one-wave kernel that closed round k - 1 (or
// opened the phase) -- then the node levels, then that kernel again: absorb the root, squeeze, record k + 1.  One linear chain.
constexpr size_t FRI_REC_STRIDE = sizeof(ExtFactor) / sizeof(uint32_t);   // words per record (the base phase uses the first)
constexpr size_t FRI_REC_WORDS = 32 * FRI_REC_STRIDE;                     // a layer has at most 2^27 elements: fewer than 32 rounds
static int commit_phase_transcript(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size, size_t words,
                                   const uint8_t* d_salts, toyni_transcript* d_tr, uint32_t* d_layers, uint8_t* d_levels, uint32_t* d_betas,
                                   hipStream_t s) {
    const bool ext = words == 4;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    if (int rc = grow(c, s, (void**)&sc.d_fri_rec, &sc.fri_rec_words, FRI_REC_WORDS, sizeof(uint32_t))) return rc;
    TranscriptState* tr = transcript_of(d_tr);
    const uint32_t nsq = ext ? 4u : 1u;
    // the host constants of a record, times R^2 (transcript_factor): Ext 1 / 2 and 11 / 2; base 1 / (2 x_k), per round
    const uint32_t half_r2 = to_mont_host(to_mont_host(BB_HALF)), half11_r2 = to_mont_host(to_mont_host(bb_mul_host(BB_HALF, 11u)));
    const auto base_r2 = [](uint32_t x) { return to_mont_host(to_mont_host(bb_mul_host(BB_HALF, bb_inv_host(x)))); };
    const uint32_t* cur = d_layer0;
    uint32_t* out = d_layers;
    uint8_t* levels = d_levels;
    const uint8_t* salts = d_salts;
    uint32_t* betas = d_betas;
    uint32_t x = x0;
    uint32_t* rec = sc.d_fri_rec;
    // From the first round whose folded layer has at most 2^TOYNI_FRI_TAIL_LOG leaves (default 9 = MERKLE_TAIL, the largest possible;
    // -1 = never: A/B runs), one workgroup runs all remaining rounds (fri_tail_rounds_kernel); it squeezes its own first beta.
    static const int tail_log = std::min(env_int("TOYNI_FRI_TAIL_LOG", 9), ilog2(MERKLE_TAIL));
    const size_t tail_leaves = tail_log < 0 ? 0 : (size_t)1 << tail_log;
    size_t m = m0;
    if ((m >> 1) > tail_leaves)
        hipLaunchKernelGGL(fri_transcript_round_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, tr, static_cast<const uint8_t*>(nullptr), nsq,
                           ext ? half_r2 : base_r2(x), half11_r2, rec, betas);
    for (; m > final_size && (m >> 1) > tail_leaves; m >>= 1) {
        const size_t half = m >> 1;
        const bool last = half == final_size;
        const size_t digests = toyni_merkle_total_digests(half);
        const uint4* round_salts = reinterpret_cast<const uint4*>(last ? nullptr : salts);
        Digest* leaves = reinterpret_cast<Digest*>(levels);
        FoldArgs f{};
        f.evals = cur;
        f.out = out;
        f.dom = sub_domain(c->plan, c->d_inv, c->plan.log_n - ilog2(m));
        f.half = half;
        const dim3 grid(grid_for(half)), block(256);
        if (ext) {
            f.coef = to_mont_host(bb_inv_host(x));
            const ExtFactor* r = reinterpret_cast<const ExtFactor*>(rec);
            if (round_salts) hipLaunchKernelGGL((fri_fold_ext_commit_rec_kernel<true>), grid, block, 0, s, f, r, round_salts, leaves);
            else hipLaunchKernelGGL((fri_fold_ext_commit_rec_kernel<false>), grid, block, 0, s, f, r, round_salts, leaves);
        } else {
            hipLaunchKernelGGL(fri_fold_commit_rec_kernel, grid, block, 0, s, f, (const uint32_t*)rec, round_salts, leaves);
        }
        if (int rc = enqueue_merkle_upper(levels, half, s)) return rc;
        const uint8_t* root = levels + (digests - 1) * 32;
        cur = out;
        out += half * words;
        levels += digests * 32;
        if (salts && !last) salts += half * 16;
        if (betas) betas += nsq;
        x = bb_mul_host(x, x);   // the squared domain of the next layer, src/fibonacci.rs:228-231
        rec += FRI_REC_STRIDE;
        const bool tail_next = (half >> 1) <= tail_leaves;   // the fused rounds squeeze for themselves
        hipLaunchKernelGGL(fri_transcript_round_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, tr, root, last || tail_next ? 0u : nsq,
                           ext ? half_r2 : base_r2(x), half11_r2, rec, betas);
    }
    if (m > final_size) {
        FriTailArgs a{};
        a.cur = cur;
        a.out = out;
        a.levels = reinterpret_cast<Digest*>(levels);
        a.salts = reinterpret_cast<const uint4*>(salts);
        a.tr = tr;
        a.betas = betas;
        a.dom = sub_domain(c->plan, c->d_inv, c->plan.log_n - ilog2(m));
        a.m = (uint32_t)m;
        a.final_size = (uint32_t)final_size;
        a.xinvR = to_mont_host(bb_inv_host(x));
        a.half_r2 = half_r2;
        a.half11_r2 = half11_r2;
        if (ext) hipLaunchKernelGGL((fri_tail_rounds_kernel<true>), dim3(1), dim3(MERKLE_TAIL_T), 0, s, a);
        else hipLaunchKernelGGL((fri_tail_rounds_kernel<false>), dim3(1), dim3(MERKLE_TAIL_T), 0, s, a);
    }
    return (int)hipGetLastError();
}

int toyni_fri_commit_phase_transcript_device(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                             const uint8_t* d_salts, toyni_transcript* d_tr, uint32_t* d_layers, uint8_t* d_levels,
                                             uint32_t* d_betas, void* stream) {
    if (!c || !d_layer0 || !d_tr || !d_layers || !d_levels) return TOYNI_E_NULL;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1 || m0 > c->n) return TOYNI_E_INVALID_SIZE;
    if (x0 == 0 || x0 >= BB_P) return TOYNI_E_RANGE;
    if (((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15) || ((uintptr_t)d_tr & 15) || ((uintptr_t)d_betas & 3)) return TOYNI_E_RANGE;
    if (m0 <= final_size) return TOYNI_OK;
    return commit_phase_transcript(c, d_layer0, m0, x0, final_size, 1, d_salts, d_tr, d_layers, d_levels, d_betas, (hipStream_t)stream);
}

int toyni_fri_commit_phase_transcript_ext_device(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                                 const uint8_t* d_salts, toyni_transcript* d_tr, uint32_t* d_layers, uint8_t* d_levels,
                                                 uint32_t* d_betas, void* stream) {
    if (!c || !d_layer0 || !d_tr || !d_layers || !d_levels) return TOYNI_E_NULL;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1) return TOYNI_E_INVALID_SIZE;
    if (x0 == 0) return TOYNI_E_ZERO_INVERSE;
    if (x0 >= BB_P) return TOYNI_E_RANGE;
    if ((((uintptr_t)d_layer0 | (uintptr_t)d_layers | (uintptr_t)d_levels | (uintptr_t)d_salts | (uintptr_t)d_tr) & 15) || ((uintptr_t)d_betas & 3))
        return TOYNI_E_RANGE;
    if (m0 > c->n) return TOYNI_E_INVALID_SIZE;
    if (m0 <= final_size) return TOYNI_OK;
    return commit_phase_transcript(c, d_layer0, m0, x0, final_size, 4, d_salts, d_tr, d_layers, d_levels, d_betas, (hipStream_t)stream);
}

// ---- the batch dimension of the tail (include/toyni_hip.h 3r) ----
// Order of the refusals in every call: null pointers, batch, the single call's own in the single call's order, the strides.
constexpr size_t BATCH_MAX = 65535;   // the proof index is a block coordinate: gridDim.y
static bool batch_ok(size_t batch) { return batch >= 1 && batch <= BATCH_MAX; }

// The levels above the leaf hashes in every proof's tree; the tree starts `at` digests into the proof's region.  A level takes the
// two-wave node hash when batch x nodes -- what the launch spreads over the chip -- is at most 2^TOYNI_MERKLE_COOP_LOG.
static int enqueue_merkle_upper_batch(uint8_t* d_levels, size_t level_stride, size_t at, size_t n, size_t batch, hipStream_t s) {
    static const int coop_log = env_int("TOYNI_MERKLE_COOP_LOG", 14);
    size_t m = n;
    const unsigned by = (unsigned)batch;
    while (m > MERKLE_TAIL) {
        const size_t up = (m + 1) / 2;
        if (coop_log >= 0 && up * batch <= ((size_t)1 << coop_log))
            hipLaunchKernelGGL(merkle_level_coop_batch_kernel, dim3((unsigned)((up + 63) / 64), by), dim3(128), 0, s, d_levels, level_stride, at, m, up);
        else
            hipLaunchKernelGGL(merkle_level_batch_kernel, dim3(grid_for(up), by), dim3(256), 0, s, d_levels, level_stride, at, m, up);
        at += m;
        m = up;
    }
    if (m > 1) hipLaunchKernelGGL(merkle_tail_batch_kernel, dim3(by), dim3(MERKLE_TAIL_T), 0, s, d_levels, level_stride, at, (uint32_t)m);
    return (int)hipGetLastError();
}

int toyni_merkle_commit_batch_device(const uint32_t* d_values, size_t value_stride, const uint8_t* d_salts, size_t salt_stride, size_t n, size_t batch,
                                     uint8_t* d_levels, size_t level_stride, void* stream) {
    if (!d_values || !d_levels) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (n == 0) return TOYNI_OK;
    if (((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15)) return TOYNI_E_RANGE;  // 16-byte accesses
    if (value_stride < n || (d_salts && (salt_stride < n * 16 || (salt_stride & 15)))) return TOYNI_E_RANGE;
    if (level_stride < toyni_merkle_total_digests(n) * 32 || (level_stride & 15)) return TOYNI_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(merkle_leaf_batch_kernel, dim3(grid_for(n), (unsigned)batch), dim3(256), 0, s, d_values, value_stride, d_salts, salt_stride, d_levels,
                       level_stride, n);
    return enqueue_merkle_upper_batch(d_levels, level_stride, 0, n, batch, s);
}

int toyni_transcript_absorb_batch_device(toyni_transcript* d_tr, size_t batch, const uint8_t* d_bytes, size_t byte_stride, size_t len, void* stream) {
    if (!d_tr || (!d_bytes && len)) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (((uintptr_t)d_tr & 15) || len > TOYNI_TRANSCRIPT_CAPACITY) return TOYNI_E_RANGE;
    if (byte_stride < len) return TOYNI_E_RANGE;
    if (len == 0) return TOYNI_OK;
    hipLaunchKernelGGL(transcript_absorb_batch_kernel, dim3((unsigned)batch), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr), d_bytes,
                       byte_stride, (uint32_t)len);
    return (int)hipGetLastError();
}

int toyni_transcript_squeeze_indices_batch_device(toyni_transcript* d_tr, size_t batch, size_t count, uint32_t max, uint32_t* d_out, size_t out_stride,
                                                  void* stream) {
    if (!d_tr || !d_out) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_out & 3)) return TOYNI_E_RANGE;
    if (count == 0 || count > TRANSCRIPT_MAX_INDICES || max == 0 || count > max) return TOYNI_E_RANGE;
    if (out_stride < count) return TOYNI_E_RANGE;
    hipLaunchKernelGGL(transcript_squeeze_indices_batch_kernel, dim3((unsigned)batch), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr),
                       (uint32_t)count, max, d_out, out_stride);
    return (int)hipGetLastError();
}

int toyni_fri_query_positions_batch_device(const uint32_t* d_indices, size_t index_stride, size_t count, size_t m0, size_t final_size, size_t batch,
                                           uint32_t* d_out, size_t out_stride, void* stream) {
    if (!d_indices || !d_out) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (((uintptr_t)d_indices & 3) || ((uintptr_t)d_out & 3)) return TOYNI_E_RANGE;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1 || (uint64_t)m0 > ((uint64_t)1 << 32) || count > 65536) return TOYNI_E_RANGE;
    const uint64_t total = m0 > final_size ? (uint64_t)(ilog2(m0) - ilog2(final_size)) * 2u * count : 0;
    if (index_stride < count || out_stride < total) return TOYNI_E_RANGE;
    if (total == 0) return TOYNI_OK;
    hipLaunchKernelGGL(fri_query_positions_batch_kernel, dim3(grid_for(total), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, d_indices, index_stride,
                       (uint32_t)count, (uint64_t)m0, total, d_out, out_stride);
    return (int)hipGetLastError();
}

// The strides of a batched phase (include/toyni_hip.h 3r): words, bytes, words, bytes, words.
struct PhaseStrides { size_t layer0, salts, layers, levels, betas; };
// a proof's extents under the sizes the entry point has accepted (m0 >= final_size, both powers of two)
static bool phase_strides_ok(const PhaseStrides& st, size_t m0, size_t final_size, size_t words, bool salted, bool betas) {
    const size_t rounds = m0 > final_size ? (size_t)(ilog2(m0) - ilog2(final_size)) : 0;
    size_t digests = 0;
    for (size_t m = m0; m > final_size; m >>= 1) digests += toyni_merkle_total_digests(m >> 1);
    const size_t folded = m0 > final_size ? m0 - final_size : 0;                      // m0 / 2 + ... + final_size elements
    const size_t salted_leaves = folded > final_size ? folded - final_size : 0;       // every folded layer but the final one
    if (st.layer0 < m0 * words || st.layers < folded * words || st.levels < digests * 32 || (st.levels & 15)) return false;
    if (words == 4 && ((st.layer0 | st.layers) & 3)) return false;                    // the Ext call's 16-byte layers
    if (salted && (st.salts < salted_leaves * 16 || (st.salts & 15))) return false;
    if (betas && st.betas < rounds * words) return false;
    return true;
}

// commit_phase_transcript with `batch` proofs per launch: the same chain, round k reading records k * batch .. k * batch + batch - 1.
static int commit_phase_transcript_batch(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size, size_t words,
                                         const uint8_t* d_salts, toyni_transcript* d_tr, size_t batch, uint32_t* d_layers, uint8_t* d_levels,
                                         uint32_t* d_betas, const PhaseStrides& st, hipStream_t s) {
    const bool ext = words == 4;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    const size_t rounds = (size_t)(ilog2(m0) - ilog2(final_size));
    if (int rc = grow(c, s, (void**)&sc.d_fri_rec, &sc.fri_rec_words, std::max(FRI_REC_WORDS, (rounds + 1) * batch * FRI_REC_STRIDE), sizeof(uint32_t)))
        return rc;
    TranscriptState* tr = transcript_of(d_tr);
    const unsigned by = (unsigned)batch;
    const uint32_t nsq = ext ? 4u : 1u;
    const uint32_t half_r2 = to_mont_host(to_mont_host(BB_HALF)), half11_r2 = to_mont_host(to_mont_host(bb_mul_host(BB_HALF, 11u)));
    const auto base_r2 = [](uint32_t x) { return to_mont_host(to_mont_host(bb_mul_host(BB_HALF, bb_inv_host(x)))); };
    // proof 0's pointers; `in_stride` is layer 0's stride in the first round and the folded layers' afterwards
    const uint32_t* cur = d_layer0;
    size_t in_stride = st.layer0;
    uint32_t* out = d_layers;
    size_t level_at = 0;               // digests into a proof's d_levels
    const uint8_t* salts = d_salts;
    uint32_t* betas = d_betas;
    uint32_t x = x0;
    uint32_t* rec = sc.d_fri_rec;
    static const int tail_log = std::min(env_int("TOYNI_FRI_TAIL_LOG", 9), ilog2(MERKLE_TAIL));
    const size_t tail_leaves = tail_log < 0 ? 0 : (size_t)1 << tail_log;
    size_t m = m0;
    if ((m >> 1) > tail_leaves)
        hipLaunchKernelGGL(fri_transcript_round_batch_kernel, dim3(by), dim3(TRANSCRIPT_T), 0, s, tr, static_cast<const uint8_t*>(nullptr), (size_t)0, nsq,
                           ext ? half_r2 : base_r2(x), half11_r2, rec, (uint32_t)FRI_REC_STRIDE, betas, st.betas);
    for (; m > final_size && (m >> 1) > tail_leaves; m >>= 1) {
        const size_t half = m >> 1;
        const bool last = half == final_size;
        const size_t digests = toyni_merkle_total_digests(half);
        const uint8_t* round_salts = last ? nullptr : salts;
        uint8_t* leaves = d_levels + level_at * 32;
        FoldArgs f{};
        f.evals = cur;
        f.out = out;
        f.dom = sub_domain(c->plan, c->d_inv, c->plan.log_n - ilog2(m));
        f.half = half;
        const FoldBatch fb{in_stride, st.layers, st.salts, st.levels, (uint32_t)FRI_REC_STRIDE};
        const dim3 grid(grid_for(half), by), block(256);
        if (ext) {
            f.coef = to_mont_host(bb_inv_host(x));
            if (round_salts) hipLaunchKernelGGL((fri_fold_ext_commit_rec_batch_kernel<true>), grid, block, 0, s, f, fb, (const uint32_t*)rec, round_salts, leaves);
            else hipLaunchKernelGGL((fri_fold_ext_commit_rec_batch_kernel<false>), grid, block, 0, s, f, fb, (const uint32_t*)rec, round_salts, leaves);
        } else {
            hipLaunchKernelGGL(fri_fold_commit_rec_batch_kernel, grid, block, 0, s, f, fb, (const uint32_t*)rec, round_salts, leaves);
        }
        if (int rc = enqueue_merkle_upper_batch(d_levels, st.levels, level_at, half, batch, s)) return rc;
        const uint8_t* root = d_levels + (level_at + digests - 1) * 32;
        cur = out;
        in_stride = st.layers;
        out += half * words;
        level_at += digests;
        if (salts && !last) salts += half * 16;
        if (betas) betas += nsq;
        x = bb_mul_host(x, x);
        rec += batch * FRI_REC_STRIDE;
        const bool tail_next = (half >> 1) <= tail_leaves;
        hipLaunchKernelGGL(fri_transcript_round_batch_kernel, dim3(by), dim3(TRANSCRIPT_T), 0, s, tr, root, st.levels, last || tail_next ? 0u : nsq,
                           ext ? half_r2 : base_r2(x), half11_r2, rec, (uint32_t)FRI_REC_STRIDE, betas, st.betas);
    }
    if (m > final_size) {
        FriTailArgs a{};
        a.cur = cur;
        a.out = out;
        a.levels = reinterpret_cast<Digest*>(d_levels + level_at * 32);
        a.salts = reinterpret_cast<const uint4*>(salts);
        a.tr = tr;
        a.betas = betas;
        a.dom = sub_domain(c->plan, c->d_inv, c->plan.log_n - ilog2(m));
        a.m = (uint32_t)m;
        a.final_size = (uint32_t)final_size;
        a.xinvR = to_mont_host(bb_inv_host(x));
        a.half_r2 = half_r2;
        a.half11_r2 = half11_r2;
        const FriTailBatch tb{in_stride, st.layers, st.levels, st.salts, st.betas};
        if (ext) hipLaunchKernelGGL((fri_tail_rounds_batch_kernel<true>), dim3(by), dim3(MERKLE_TAIL_T), 0, s, a, tb);
        else hipLaunchKernelGGL((fri_tail_rounds_batch_kernel<false>), dim3(by), dim3(MERKLE_TAIL_T), 0, s, a, tb);
    }
    return (int)hipGetLastError();
}

int toyni_fri_commit_phase_transcript_batch_device(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t layer0_stride, size_t m0, uint32_t x0,
                                                   size_t final_size, const uint8_t* d_salts, size_t salt_stride, toyni_transcript* d_tr, size_t batch,
                                                   uint32_t* d_layers, size_t layers_stride, uint8_t* d_levels, size_t level_stride, uint32_t* d_betas,
                                                   size_t beta_stride, void* stream) {
    if (!c || !d_layer0 || !d_tr || !d_layers || !d_levels) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1 || m0 > c->n) return TOYNI_E_INVALID_SIZE;
    if (x0 == 0 || x0 >= BB_P) return TOYNI_E_RANGE;
    if (((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15) || ((uintptr_t)d_tr & 15) || ((uintptr_t)d_betas & 3)) return TOYNI_E_RANGE;
    const PhaseStrides st{layer0_stride, salt_stride, layers_stride, level_stride, beta_stride};
    if (!phase_strides_ok(st, m0, final_size, 1, d_salts != nullptr, d_betas != nullptr)) return TOYNI_E_RANGE;
    if (m0 <= final_size) return TOYNI_OK;
    return commit_phase_transcript_batch(c, d_layer0, m0, x0, final_size, 1, d_salts, d_tr, batch, d_layers, d_levels, d_betas, st, (hipStream_t)stream);
}

int toyni_fri_commit_phase_transcript_ext_batch_device(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t layer0_stride, size_t m0, uint32_t x0,
                                                       size_t final_size, const uint8_t* d_salts, size_t salt_stride, toyni_transcript* d_tr, size_t batch,
                                                       uint32_t* d_layers, size_t layers_stride, uint8_t* d_levels, size_t level_stride,
                                                       uint32_t* d_betas, size_t beta_stride, void* stream) {
    if (!c || !d_layer0 || !d_tr || !d_layers || !d_levels) return TOYNI_E_NULL;
    if (!batch_ok(batch)) return TOYNI_E_RANGE;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1) return TOYNI_E_INVALID_SIZE;
    if (x0 == 0) return TOYNI_E_ZERO_INVERSE;
    if (x0 >= BB_P) return TOYNI_E_RANGE;
    if ((((uintptr_t)d_layer0 | (uintptr_t)d_layers | (uintptr_t)d_levels | (uintptr_t)d_salts | (uintptr_t)d_tr) & 15) || ((uintptr_t)d_betas & 3))
        return TOYNI_E_RANGE;
    if (m0 > c->n) return TOYNI_E_INVALID_SIZE;
    const PhaseStrides st{layer0_stride, salt_stride, layers_stride, level_stride, beta_stride};
    if (!phase_strides_ok(st, m0, final_size, 4, d_salts != nullptr, d_betas != nullptr)) return TOYNI_E_RANGE;
    if (m0 <= final_size) return TOYNI_OK;
    return commit_phase_transcript_batch(c, d_layer0, m0, x0, final_size, 4, d_salts, d_tr, batch, d_layers, d_levels, d_betas, st, (hipStream_t)stream);
}

// ---- four-to-one Ext FRI rounds under coset leaves (include/toyni_hip.h 3m) ----
int toyni_merkle_commit_cosets_ext_device(const uint32_t* d_layer, size_t m, const uint8_t* d_salts, uint8_t* d_levels, void* stream) {
    if (!d_layer || !d_levels) return TOYNI_E_NULL;
    if (m == 0) return TOYNI_OK;
    if (!is_pow2(m) || m < 4) return TOYNI_E_INVALID_SIZE;
    if (m > ((size_t)1 << 33) || (((uintptr_t)d_layer | (uintptr_t)d_levels | (uintptr_t)d_salts) & 15)) return TOYNI_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = m / 4;
    const uint4* salts = reinterpret_cast<const uint4*>(d_salts);
    Digest* out = reinterpret_cast<Digest*>(d_levels);
    const dim3 grid(grid_for(n)), block(256);
    if (salts) hipLaunchKernelGGL((merkle_coset_leaf_kernel<true>), grid, block, 0, s, d_layer, salts, out, n);
    else hipLaunchKernelGGL((merkle_coset_leaf_kernel<false>), grid, block, 0, s, d_layer, salts, out, n);
    return enqueue_merkle_upper(d_levels, n, s);
}

int toyni_merkle_open_cosets_ext_device(const uint8_t* d_levels, size_t m, const uint32_t* d_layer, const uint8_t* d_salts, const uint32_t* d_indices,
                                        size_t nidx, uint8_t* d_out, void* stream) {
    if (!d_levels || !d_layer || !d_indices || !d_out) return TOYNI_E_NULL;
    if (m == 0) return TOYNI_OK;
    if (!is_pow2(m) || m < 4) return TOYNI_E_INVALID_SIZE;
    if (m > ((size_t)1 << 33) || nidx > 0xFFFFFFFFull || (((uintptr_t)d_levels | (uintptr_t)d_layer | (uintptr_t)d_salts) & 15) ||
        ((uintptr_t)d_out & 7) || ((uintptr_t)d_indices & 3)) return TOYNI_E_RANGE;
    if (nidx == 0) return TOYNI_OK;
    const size_t n = m / 4;
    const uint64_t work = (uint64_t)nidx * (merkle_depth(n) + 1 + 16);
    const OpenRows g{reinterpret_cast<const Digest*>(d_levels), (uint64_t)n, d_layer, 16u, ROWS_EXT_QUARTERS, (uint64_t)n,
                     reinterpret_cast<const uint4*>(d_salts), d_indices, (uint32_t)nidx, d_out};
    hipLaunchKernelGGL(merkle_open_cosets_kernel, dim3(grid_for(work)), dim3(256), 0, (hipStream_t)stream, g);
    return (int)hipGetLastError();
}

// beta^2 / 2 on the host (src/ext.rs:178-192), for the call that is handed beta
static ExtFactor ext_square_half_host(const uint32_t b[4]) {
    const auto mul = bb_mul_host;
    const auto add = [](uint32_t x, uint32_t y) { return (uint32_t)(((uint64_t)x + y) % BB_P); };
    uint32_t sq[4];
    sq[0] = add(mul(b[0], b[0]), mul(11u, add(add(mul(b[1], b[3]), mul(b[2], b[2])), mul(b[3], b[1]))));
    sq[1] = add(add(mul(b[0], b[1]), mul(b[1], b[0])), mul(11u, add(mul(b[2], b[3]), mul(b[3], b[2]))));
    sq[2] = add(add(mul(b[0], b[2]), mul(b[1], b[1])), add(mul(b[2], b[0]), mul(11u, mul(b[3], b[3]))));
    sq[3] = add(add(mul(b[0], b[3]), mul(b[1], b[2])), add(mul(b[2], b[1]), mul(b[3], b[0])));
    ExtFactor f{};
    ext_beta_half(sq, &f);
    return f;
}

// Arguments checked by the caller: m >= 16 a power of two <= n, x in [1, p).
static Fold4ExtArgs fold4_args(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, uint32_t x) {
    Fold4ExtArgs a{};
    a.evals = d_evals;
    a.out = d_out;
    a.dom = sub_domain(c->plan, c->d_inv, c->plan.log_n - ilog2(m));
    a.xinvR = to_mont_host(bb_inv_host(x));
    a.iinvR = to_mont_host(bb_inv_host(bb_root_of_unity_host(2)));
    a.leaves = m / 16;
    return a;
}

int toyni_fri_fold4_commit_ext_device(toyni_ntt_ctx* c, const uint32_t* d_evals, uint32_t* d_out, size_t m, const uint32_t beta[4], uint32_t x0,
                                      const uint8_t* d_salts, uint8_t* d_levels, void* stream) {
    // every refusal that the arguments alone decide comes before the context is read
    if (!c || !d_evals || !d_out || !beta || !d_levels) return TOYNI_E_NULL;
    if (m && (!is_pow2(m) || m < 16)) return TOYNI_E_RANGE;
    if (x0 == 0) return TOYNI_E_ZERO_INVERSE;
    if (((uintptr_t)d_evals | (uintptr_t)d_out | (uintptr_t)d_levels | (uintptr_t)d_salts) & 15) return TOYNI_E_RANGE;   // 16-byte accesses
    Fold4ExtFactors f{};
    if (x0 >= BB_P || !ext_beta_half(beta, &f.beta_half)) return TOYNI_E_RANGE;
    f.beta2_half = ext_square_half_host(beta);
    if (m == 0) return TOYNI_OK;
    if (m > c->n) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    const Fold4ExtArgs a = fold4_args(c, d_evals, d_out, m, x0);
    const dim3 grid(grid_for(a.leaves)), block(256);
    Digest* leaves = reinterpret_cast<Digest*>(d_levels);
    if (d_salts) hipLaunchKernelGGL((fri_fold4_ext_commit_kernel<true>), grid, block, 0, s, a, f, reinterpret_cast<const uint4*>(d_salts), leaves);
    else hipLaunchKernelGGL((fri_fold4_ext_commit_kernel<false>), grid, block, 0, s, a, f, static_cast<const uint4*>(nullptr), leaves);
    return enqueue_merkle_upper(d_levels, a.leaves, s);
}

// log2(m0 / final_size) / 2 for sizes the four-to-one calls accept, -1 otherwise (both powers of two, final_size >= 4, an even ratio)
static int fri4_rounds(size_t m0, size_t final_size) {
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 4) return -1;
    if (m0 <= final_size) return 0;
    const int d = ilog2(m0) - ilog2(final_size);
    return d % 2 ? -1 : d / 2;
}

int toyni_fri4_query_positions_device(const uint32_t* d_indices, size_t count, size_t m0, size_t final_size, uint32_t* d_out, void* stream) {
    if (!d_indices || !d_out) return TOYNI_E_NULL;
    if (((uintptr_t)d_indices & 3) || ((uintptr_t)d_out & 3)) return TOYNI_E_RANGE;
    if (!is_pow2(m0) || !is_pow2(final_size) || final_size < 1 || (uint64_t)m0 > ((uint64_t)1 << 32) || count > 65536) return TOYNI_E_RANGE;
    const int rounds = fri4_rounds(m0, final_size);
    if (rounds < 0) return TOYNI_E_INVALID_SIZE;
    if (count == 0 || rounds == 0) return TOYNI_OK;
    const uint64_t total = (uint64_t)rounds * count;
    hipLaunchKernelGGL(fri4_query_positions_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, d_indices, (uint32_t)count, (uint64_t)m0,
                       total, d_out);
    return (int)hipGetLastError();
}

// The phase: the chain of commit_phase_transcript with half the rounds and no fused tail -- per round the fold (its record written by
// the one-wave kernel that closed the round before, or opened the phase), the node levels, that kernel again.  A record is 16 words:
// at most 13 rounds (2^27 down to 4) fit the FRI_REC_WORDS buffer of the stream.
static_assert(13 * sizeof(Fold4ExtFactors) <= FRI_REC_WORDS * sizeof(uint32_t), "the four-to-one records fit the stream's record buffer");
int toyni_fri4_commit_phase_transcript_ext_device(toyni_ntt_ctx* c, const uint32_t* d_layer0, size_t m0, uint32_t x0, size_t final_size,
                                                  const uint8_t* d_salts, toyni_transcript* d_tr, uint32_t* d_layers, uint8_t* d_levels,
                                                  uint32_t* d_betas, void* stream) {
    if (!c || !d_layer0 || !d_tr || !d_layers || !d_levels) return TOYNI_E_NULL;
    if (fri4_rounds(m0, final_size) < 0) return TOYNI_E_INVALID_SIZE;
    if (x0 == 0) return TOYNI_E_ZERO_INVERSE;
    if (x0 >= BB_P) return TOYNI_E_RANGE;
    if ((((uintptr_t)d_layer0 | (uintptr_t)d_layers | (uintptr_t)d_levels | (uintptr_t)d_salts | (uintptr_t)d_tr) & 15) || ((uintptr_t)d_betas & 3))
        return TOYNI_E_RANGE;
    if (m0 > c->n) return TOYNI_E_INVALID_SIZE;
    if (m0 <= final_size) return TOYNI_OK;
    hipStream_t s = (hipStream_t)stream;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    if (int rc = grow(c, s, (void**)&sc.d_fri_rec, &sc.fri_rec_words, FRI_REC_WORDS, sizeof(uint32_t))) return rc;
    TranscriptState* tr = transcript_of(d_tr);
    const uint32_t half_r2 = to_mont_host(to_mont_host(BB_HALF)), half11_r2 = to_mont_host(to_mont_host(bb_mul_host(BB_HALF, 11u)));
    const uint32_t eleven_r2 = to_mont_host(to_mont_host(11u));
    const uint32_t* cur = d_layer0;
    uint32_t* out = d_layers;
    uint8_t* levels = d_levels;
    const uint8_t* salts = d_salts;
    uint32_t* betas = d_betas;
    uint32_t x = x0;
    uint32_t* rec = sc.d_fri_rec;
    hipLaunchKernelGGL(fri4_transcript_round_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, tr, static_cast<const uint8_t*>(nullptr), 1u, half_r2, half11_r2,
                       eleven_r2, rec, betas);
    for (size_t m = m0; m > final_size; m >>= 2) {
        const size_t quarter = m >> 2;
        const bool last = quarter == final_size;
        const Fold4ExtArgs a = fold4_args(c, cur, out, m, x);
        const size_t digests = toyni_merkle_total_digests(a.leaves);
        const uint4* round_salts = reinterpret_cast<const uint4*>(last ? nullptr : salts);
        Digest* leaves = reinterpret_cast<Digest*>(levels);
        const Fold4ExtFactors* r = reinterpret_cast<const Fold4ExtFactors*>(rec);
        const dim3 grid(grid_for(a.leaves)), block(256);
        if (round_salts) hipLaunchKernelGGL((fri_fold4_ext_commit_rec_kernel<true>), grid, block, 0, s, a, r, round_salts, leaves);
        else hipLaunchKernelGGL((fri_fold4_ext_commit_rec_kernel<false>), grid, block, 0, s, a, r, round_salts, leaves);
        if (int rc = enqueue_merkle_upper(levels, a.leaves, s)) return rc;
        const uint8_t* root = levels + (digests - 1) * 32;
        cur = out;
        out += quarter * 4;
        levels += digests * 32;
        if (salts && !last) salts += a.leaves * 16;
        if (betas) betas += 4;
        x = bb_mul_host(x, x);
        x = bb_mul_host(x, x);   // x^4: the domain of the next layer
        rec += sizeof(Fold4ExtFactors) / sizeof(uint32_t);
        hipLaunchKernelGGL(fri4_transcript_round_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, tr, root, last ? 0u : 1u, half_r2, half11_r2, eleven_r2, rec,
                           betas);
    }
    return (int)hipGetLastError();
}

static DomainArgs domain_args(toyni_ntt_ctx* c, unsigned log_m, uint32_t shift) {
    DomainArgs d{};
    d.dom = sub_domain(c->plan, c->d_fwd, c->plan.log_n - (int)log_m);
    d.shiftR = to_mont_host(shift);
    return d;
}

int toyni_fib_quotient_device(toyni_ntt_ctx* c, const uint32_t* d_trace_lde, uint32_t* d_c_evals, uint32_t* d_q_evals, unsigned log_blowup,
                              uint32_t shift, void* stream) {
    if (!c || !d_trace_lde || !d_q_evals) return TOYNI_E_NULL;
    const int log_N = c->plan.log_n;
    if ((int)log_blowup > log_N || log_blowup > 10 || shift == 0 || shift >= BB_P) return TOYNI_E_RANGE;
    const int log_n = log_N - (int)log_blowup;
    if (log_n < 1) return TOYNI_E_RANGE;                                    // the AIR needs a trace of at least two rows
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    QuotientArgs a{};
    a.trace = d_trace_lde;
    a.c_out = d_c_evals;
    a.q_out = d_q_evals;
    a.dom = domain_args(c, (unsigned)log_N, shift);
    a.log_N = (uint32_t)log_N;
    a.log_blowup = log_blowup;
    const uint64_t n = 1ull << log_n;
    const uint32_t g = bb_root_of_unity_host((uint32_t)log_n);                // domain.group_gen(), src/fibonacci.rs:108
    a.b1R = to_mont_host(bb_pow_host(g, n - 1));
    a.b2R = to_mont_host(bb_pow_host(g, n - 2));
    a.shift_nR = to_mont_host(bb_pow_host(shift, n));
    a.wBR = to_mont_host(bb_pow_host(bb_root_of_unity_host((uint32_t)log_N), n));
    // Z_H(x) = 0 on the coset only if shift^n is a B-th root of unity: then the quotient does not exist (the reference divides by zero)
    {
        uint32_t t = bb_pow_host(shift, n);
        if (bb_pow_host(t, 1ull << log_blowup) == 1u) return TOYNI_E_ZERO_INVERSE;
    }
    const bool quads = log_blowup >= 2 && log_N >= 2 && !(((uintptr_t)d_trace_lde | (uintptr_t)d_c_evals | (uintptr_t)d_q_evals) & 15);
    const uint64_t items = quads ? (1ull << log_N) / 4 : (1ull << log_N);   // (the kernel makes the same choice)
    hipLaunchKernelGGL(fib_quotient_kernel, dim3(grid_for(items)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int toyni_fib_deep_device(toyni_ntt_ctx* c, const uint32_t* d_trace_lde, const uint32_t* d_q_evals, uint32_t* d_out, unsigned log_blowup,
                          uint32_t shift, uint32_t z, const uint32_t ood[4], void* stream) {
    if (!c || !d_trace_lde || !d_q_evals || !d_out || !ood) return TOYNI_E_NULL;
    const int log_N = c->plan.log_n;
    if ((int)log_blowup > log_N || shift == 0 || shift >= BB_P || z >= BB_P) return TOYNI_E_RANGE;
    for (int k = 0; k < 4; ++k) if (ood[k] >= BB_P) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    DeepArgs a{};
    a.trace = d_trace_lde;
    a.quot = d_q_evals;
    a.out = d_out;
    a.dom = domain_args(c, (unsigned)log_N, shift);
    a.log_N = (uint32_t)log_N;
    a.log_blowup = log_blowup;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.zR = to_mont_host(z);
    a.t_z = ood[0]; a.t_gz = ood[1]; a.t_ggz = ood[2]; a.q_z = ood[3];
    const uint64_t items = log_N >= 3 ? (1ull << log_N) / 8 : (1ull << log_N);
    hipLaunchKernelGGL(fib_deep_kernel, dim3(grid_for(items)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int toyni_poly_eval_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, size_t ncoeffs, const uint32_t* points, unsigned npoints, uint32_t* d_out,
                           void* stream) {
    if (!c || !points || !d_out || (!d_coeffs && ncoeffs)) return TOYNI_E_NULL;
    if (npoints < 1 || npoints > (unsigned)POLY_MAX_POINTS) return TOYNI_E_RANGE;
    for (unsigned p = 0; p < npoints; ++p) if (points[p] >= BB_P) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (ncoeffs == 0) return (int)hipMemsetAsync(d_out, 0, npoints * sizeof(uint32_t), s);  // the zero polynomial, polynomial.rs:135-137
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    PolyEvalArgs a{};
    a.coeffs = d_coeffs;
    a.ncoeffs = ncoeffs;
    a.npoints = npoints;
    a.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, (size_t)a.nblocks * npoints, sizeof(uint32_t));
    if (rc) return rc;
    a.partial = sc.d_lde32;
    a.out = d_out;
    for (unsigned p = 0; p < npoints; ++p) {
        a.zR[p] = to_mont_host(points[p]);
        a.z16R[p] = to_mont_host(bb_pow_host(points[p], POLY_PER_THREAD));
        a.zchunkR[p] = to_mont_host(bb_pow_host(points[p], POLY_CHUNK));
    }
    hipLaunchKernelGGL(poly_eval_partial_kernel, dim3(a.nblocks), dim3(POLY_THREADS), 0, s, a);
    hipLaunchKernelGGL(poly_eval_final_kernel, dim3(1), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

// ---- section 3e: the out-of-domain values of a whole batch, and the DEEP combination of a column-major matrix ----
int toyni_poly_eval_batch_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, size_t ncoeffs, size_t stride, size_t batch, const uint32_t* points,
                                 unsigned npoints, uint32_t* d_out, void* stream) {
    if (!c || !points || !d_out || (!d_coeffs && ncoeffs)) return TOYNI_E_NULL;
    if (npoints < 1 || npoints > (unsigned)POLY_MAX_POINTS) return TOYNI_E_RANGE;
    for (unsigned p = 0; p < npoints; ++p) if (points[p] >= BB_P) return TOYNI_E_RANGE;
    if ((batch > 1 && stride < ncoeffs) || batch > 0xFFFFFFFFull || (((uintptr_t)d_coeffs | (uintptr_t)d_out) & 3)) return TOYNI_E_RANGE;
    if (batch == 0) return TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (ncoeffs == 0) return (int)hipMemsetAsync(d_out, 0, batch * npoints * sizeof(uint32_t), s);   // zero polynomials
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    PolyBatchArgs a{};
    a.e.coeffs = d_coeffs;
    a.e.ncoeffs = ncoeffs;
    a.e.npoints = npoints;
    a.e.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    a.stride = stride;
    a.batch = (uint32_t)batch;
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, batch * a.e.nblocks * npoints, sizeof(uint32_t));
    if (rc) return rc;
    a.e.partial = sc.d_lde32;
    a.e.out = d_out;
    for (unsigned p = 0; p < npoints; ++p) {
        a.e.zR[p] = to_mont_host(points[p]);
        a.e.z16R[p] = to_mont_host(bb_pow_host(points[p], POLY_PER_THREAD));
        a.e.zchunkR[p] = to_mont_host(bb_pow_host(points[p], POLY_CHUNK));
    }
    const unsigned rows = (unsigned)std::min<size_t>(batch, 65535);
    hipLaunchKernelGGL(poly_eval_batch_partial_kernel, dim3(a.e.nblocks, rows), dim3(POLY_THREADS), 0, s, a);
    hipLaunchKernelGGL(poly_eval_batch_final_kernel, dim3(rows), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

int toyni_deep_combine_device(toyni_ntt_ctx* c, const uint32_t* d_values, size_t width, size_t col_stride, unsigned log_blowup, uint32_t shift,
                              uint32_t z, const toyni_deep_term* terms, size_t nterms, int accumulate, uint32_t* d_out, void* stream) {
    if (!c || !d_values || !d_out || (!terms && nterms)) return TOYNI_E_NULL;
    const int log_N = c->plan.log_n;
    const uint64_t N = 1ull << log_N;
    if ((int)log_blowup > log_N || shift == 0 || shift >= BB_P || z >= BB_P || width == 0 || width > 65536 || col_stride < N ||
        nterms > ((size_t)1 << 20) || (((uintptr_t)d_values | (uintptr_t)d_out) & 3))
        return TOYNI_E_RANGE;
    for (size_t t = 0; t < nterms; ++t)
        if (terms[t].column >= width || terms[t].rotation >= (N >> log_blowup) || terms[t].alpha >= BB_P || terms[t].value >= BB_P) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (nterms == 0) return accumulate ? TOYNI_OK : (int)hipMemsetAsync(d_out, 0, N * sizeof(uint32_t), s);
    // the table the kernel reads: sorted by (column, rotation) so that the rotations of one column -- B words apart, lines the
    // first of them has just fetched -- are read back to back; the claimed values collapse into one constant
    std::vector<DeepTerm> table(nterms);
    uint32_t claim = 0;
    for (size_t t = 0; t < nterms; ++t) {
        table[t] = DeepTerm{terms[t].column, (uint32_t)((uint64_t)terms[t].rotation << log_blowup), to_mont_host(terms[t].alpha), 0u};
        claim = (uint32_t)((claim + (uint64_t)terms[t].alpha * terms[t].value) % BB_P);
    }
    std::stable_sort(table.begin(), table.end(), [](const DeepTerm& x, const DeepTerm& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
    DeepCombineArgs a{};
    a.values = d_values;
    a.out = d_out;
    a.col_stride = col_stride;
    a.dom = domain_args(c, (unsigned)log_N, shift);
    a.log_N = (uint32_t)log_N;
    a.nterms = (uint32_t)nterms;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.zR = to_mont_host(z);
    a.claim = claim;
    a.accumulate = accumulate ? 1u : 0u;
    const uint64_t items = log_N >= 3 ? N / 8 : N;
    const dim3 grid((unsigned)((items + 255) / 256));
    if (nterms <= DEEP_INLINE_TERMS) {   // the table rides in the kernel arguments
        DeepInlineTerms in{};
        std::copy(table.begin(), table.end(), in.t);
        hipLaunchKernelGGL(deep_combine_inline_kernel, grid, dim3(256), 0, s, a, in);
        return (int)hipGetLastError();
    }
    // a longer table: pinned staging ring -> the stream's intermediate buffer by a stream-ordered copy (an earlier call's kernel on
    // this stream is ahead of the copy; the ring keeps the bytes alive until the copy has run)
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, nterms * (sizeof(DeepTerm) / sizeof(uint32_t)), sizeof(uint32_t));
    if (rc) return rc;
    void* h = nullptr;
    if ((rc = ring_slice(sc, s, nterms * sizeof(DeepTerm), &h))) return rc;
    std::memcpy(h, table.data(), nterms * sizeof(DeepTerm));
    HIPCHK(hipMemcpyAsync(sc.d_lde32, h, nterms * sizeof(DeepTerm), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(deep_combine_kernel, grid, dim3(256), 0, s, a, reinterpret_cast<const DeepTerm*>(sc.d_lde32));
    return (int)hipGetLastError();
}

// ---- section 3h: the same two steps under Ext challenges ----
static bool ext_canonical(const uint32_t v[4]) { return v[0] < BB_P && v[1] < BB_P && v[2] < BB_P && v[3] < BB_P; }

int toyni_poly_eval_ext_batch_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, size_t ncoeffs, size_t stride, size_t batch, const uint32_t* points,
                                     unsigned npoints, uint32_t* d_out, void* stream) {
    if (!c || !points || !d_out || (!d_coeffs && ncoeffs)) return TOYNI_E_NULL;
    if (npoints < 1 || npoints > (unsigned)POLY_MAX_POINTS) return TOYNI_E_RANGE;
    for (unsigned p = 0; p < npoints; ++p) if (!ext_canonical(points + 4 * p)) return TOYNI_E_RANGE;
    if ((batch > 1 && stride < ncoeffs) || batch > 0xFFFFFFFFull || (((uintptr_t)d_coeffs | (uintptr_t)d_out) & 3)) return TOYNI_E_RANGE;
    if (batch == 0) return TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (ncoeffs == 0) return (int)hipMemsetAsync(d_out, 0, batch * npoints * 4 * sizeof(uint32_t), s);   // zero polynomials
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    PolyExtArgs a{};
    a.coeffs = d_coeffs;
    a.ncoeffs = ncoeffs;
    a.stride = stride;
    a.batch = (uint32_t)batch;
    a.npoints = npoints;
    a.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, batch * a.nblocks * npoints * 4, sizeof(uint32_t));
    if (rc) return rc;
    a.partial = sc.d_lde32;
    a.out = d_out;
    for (unsigned p = 0; p < npoints; ++p) {
        uint32_t z16[4], zchunk[4], zstride[4];
        ext_pow_host(points + 4 * p, POLY_PER_THREAD, z16);
        ext_pow_host(points + 4 * p, POLY_CHUNK, zchunk);
        ext_pow_host(zchunk, POLY_THREADS, zstride);
        a.thread[p] = poly_ext_powers_host(points + 4 * p, z16);
        a.chunk[p] = poly_ext_powers_host(zstride, zchunk);
    }
    const unsigned rows = (unsigned)std::min<size_t>(batch, 65535);
    hipLaunchKernelGGL(poly_eval_ext_batch_partial_kernel, dim3(a.nblocks, rows), dim3(POLY_THREADS), 0, s, a);
    hipLaunchKernelGGL(poly_eval_ext_batch_final_kernel, dim3(rows), dim3(POLY_THREADS), 0, s, a);
    return (int)hipGetLastError();
}

int toyni_deep_combine_ext_device(toyni_ntt_ctx* c, const uint32_t* d_values, size_t width, size_t col_stride, unsigned log_blowup, uint32_t shift,
                                  const uint32_t z[4], const toyni_deep_ext_term* terms, size_t nterms, int accumulate, uint32_t* d_out,
                                  void* stream) {
    if (!c || !d_values || !d_out || !z || (!terms && nterms)) return TOYNI_E_NULL;
    const int log_N = c->plan.log_n;
    const uint64_t N = 1ull << log_N;
    if ((int)log_blowup > log_N || shift == 0 || shift >= BB_P || !ext_canonical(z) || width == 0 || width > 65536 || col_stride < N ||
        nterms > ((size_t)1 << 20) || ((uintptr_t)d_values & 3) || ((uintptr_t)d_out & 15))
        return TOYNI_E_RANGE;
    for (size_t t = 0; t < nterms; ++t)
        if (terms[t].column >= width || terms[t].rotation >= (N >> log_blowup) || !ext_canonical(terms[t].alpha) || !ext_canonical(terms[t].value))
            return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (nterms == 0) return accumulate ? TOYNI_OK : (int)hipMemsetAsync(d_out, 0, N * 4 * sizeof(uint32_t), s);
    // the table the kernel reads, sorted by (column, rotation) as the base call's is; the claimed values collapse into one Ext constant
    std::vector<DeepExtTerm> table(nterms);
    DeepExtArgs a{};
    for (size_t t = 0; t < nterms; ++t) {
        DeepExtTerm& e = table[t];
        e = DeepExtTerm{};
        e.column = terms[t].column;
        e.rot = (uint32_t)((uint64_t)terms[t].rotation << log_blowup);
        uint32_t av[4];
        ext_mul_host(terms[t].alpha, terms[t].value, av);
        for (int k = 0; k < 4; ++k) {
            e.alphaR[k] = to_mont_host(terms[t].alpha[k]);
            a.claim[k] = (uint32_t)(((uint64_t)a.claim[k] + av[k]) % BB_P);
        }
    }
    std::stable_sort(table.begin(), table.end(), [](const DeepExtTerm& x, const DeepExtTerm& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
    a.values = d_values;
    a.out = d_out;
    a.col_stride = col_stride;
    a.dom = domain_args(c, (unsigned)log_N, shift);
    a.log_N = (uint32_t)log_N;
    a.nterms = (uint32_t)nterms;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.accumulate = accumulate ? 1u : 0u;
    a.shift = ext_shift_host(z);
    const uint64_t items = log_N >= 2 ? N / 4 : N;
    const dim3 grid((unsigned)((items + 255) / 256));
    if (nterms <= DEEP_EXT_INLINE_TERMS) {   // the table rides in the kernel arguments
        DeepExtInlineTerms in{};
        std::copy(table.begin(), table.end(), in.t);
        hipLaunchKernelGGL(deep_combine_ext_inline_kernel, grid, dim3(256), 0, s, a, in);
        return (int)hipGetLastError();
    }
    // a longer table: pinned staging ring -> the stream's intermediate buffer by a stream-ordered copy, as toyni_deep_combine_device
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, nterms * (sizeof(DeepExtTerm) / sizeof(uint32_t)), sizeof(uint32_t));
    if (rc) return rc;
    void* h = nullptr;
    if ((rc = ring_slice(sc, s, nterms * sizeof(DeepExtTerm), &h))) return rc;
    std::memcpy(h, table.data(), nterms * sizeof(DeepExtTerm));
    HIPCHK(hipMemcpyAsync(sc.d_lde32, h, nterms * sizeof(DeepExtTerm), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(deep_combine_ext_kernel, grid, dim3(256), 0, s, a, reinterpret_cast<const DeepExtTerm*>(sc.d_lde32));
    return (int)hipGetLastError();
}

// ---- section 3o: the same two steps with z, the weights and the claimed values in device memory, and the helpers around them ----
int toyni_transcript_squeeze_ext_point_device(toyni_transcript* d_tr, uint32_t* d_z, void* stream) {
    if (!d_tr || !d_z) return TOYNI_E_NULL;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_z & 3)) return TOYNI_E_RANGE;
    hipLaunchKernelGGL(transcript_squeeze_ext_point_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr), d_z);
    return (int)hipGetLastError();
}

int toyni_transcript_absorb_fields_device(toyni_transcript* d_tr, const uint32_t* d_words, size_t count, void* stream) {
    if (!d_tr || (!d_words && count)) return TOYNI_E_NULL;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_words & 3) || count > TRANSCRIPT_MAX_FIELDS) return TOYNI_E_RANGE;
    if (count == 0) return TOYNI_OK;
    hipLaunchKernelGGL(transcript_absorb_fields_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr), d_words, (uint32_t)count);
    return (int)hipGetLastError();
}

int toyni_query_rows_device(const uint32_t* d_indices, size_t count, size_t n, const uint32_t* offsets, unsigned noffsets, uint32_t* d_out, void* stream) {
    if (!d_indices || !d_out || !offsets) return TOYNI_E_NULL;
    if (((uintptr_t)d_indices & 3) || ((uintptr_t)d_out & 3) || noffsets < 1 || noffsets > QUERY_ROWS_MAX_OFFSETS || n < 1 ||
        (uint64_t)n > ((uint64_t)1 << 32) || count > 65536)
        return TOYNI_E_RANGE;
    QueryRowOffsets off{};
    for (unsigned r = 0; r < noffsets; ++r) {
        if (offsets[r] >= n) return TOYNI_E_RANGE;
        off.v[r] = offsets[r];
    }
    if (count == 0) return TOYNI_OK;
    const uint64_t total = (uint64_t)count * noffsets;
    hipLaunchKernelGGL(query_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, d_indices, off, (uint32_t)noffsets, (uint64_t)n, total,
                       d_out);
    return (int)hipGetLastError();
}

int toyni_poly_eval_ext_batch_dz_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, size_t ncoeffs, size_t stride, size_t batch, const uint32_t* d_z,
                                        const uint32_t* mults, unsigned npoints, uint32_t* d_out, void* stream) {
    if (!c || !d_z || !mults || !d_out || (!d_coeffs && ncoeffs)) return TOYNI_E_NULL;
    if (npoints < 1 || npoints > (unsigned)POLY_MAX_POINTS) return TOYNI_E_RANGE;
    PolyDzMults m{};
    for (unsigned p = 0; p < npoints; ++p) {
        if (mults[p] >= BB_P) return TOYNI_E_RANGE;
        m.v[p] = mults[p];
    }
    if ((batch > 1 && stride < ncoeffs) || batch > 0xFFFFFFFFull || (((uintptr_t)d_coeffs | (uintptr_t)d_out | (uintptr_t)d_z) & 3)) return TOYNI_E_RANGE;
    if (batch == 0) return TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (ncoeffs == 0) return (int)hipMemsetAsync(d_out, 0, batch * npoints * 4 * sizeof(uint32_t), s);   // zero polynomials
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    PolyExtDzArgs a{};
    a.coeffs = d_coeffs;
    a.ncoeffs = ncoeffs;
    a.stride = stride;
    a.batch = (uint32_t)batch;
    a.npoints = npoints;
    a.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    // the stream's buffer: the partial sums (a multiple of four words), then the record
    const size_t partial_words = batch * a.nblocks * npoints * 4;
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, partial_words + sizeof(PolyExtRecord) / sizeof(uint32_t), sizeof(uint32_t));
    if (rc) return rc;
    a.partial = sc.d_lde32;
    a.out = d_out;
    PolyExtRecord* rec = reinterpret_cast<PolyExtRecord*>(sc.d_lde32 + partial_words);
    hipLaunchKernelGGL(poly_ext_prepare_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, d_z, m, (uint32_t)npoints, rec);
    const unsigned rows = (unsigned)std::min<size_t>(batch, 65535);
    hipLaunchKernelGGL(poly_eval_ext_batch_partial_dz_kernel, dim3(a.nblocks, rows), dim3(POLY_THREADS), 0, s, a,
                       static_cast<const PolyExtRecord*>(rec));
    hipLaunchKernelGGL(poly_eval_ext_batch_final_dz_kernel, dim3(rows), dim3(POLY_THREADS), 0, s, a, static_cast<const PolyExtRecord*>(rec));
    return (int)hipGetLastError();
}

int toyni_deep_combine_ext_dz_device(toyni_ntt_ctx* c, const uint32_t* d_values, size_t width, size_t col_stride, unsigned log_blowup, uint32_t shift,
                                     const uint32_t* d_z, const uint32_t* d_alphas, const uint32_t* d_claims, const toyni_deep_ext_slot* slots,
                                     size_t nslots, int accumulate, uint32_t* d_out, void* stream) {
    if (!c || !d_values || !d_out || !d_z || !d_alphas || !d_claims || (!slots && nslots)) return TOYNI_E_NULL;
    const int log_N = c->plan.log_n;
    const uint64_t N = 1ull << log_N;
    if ((int)log_blowup > log_N || shift == 0 || shift >= BB_P || width == 0 || width > 65536 || col_stride < N || nslots > ((size_t)1 << 20) ||
        (((uintptr_t)d_values | (uintptr_t)d_z | (uintptr_t)d_alphas | (uintptr_t)d_claims) & 3) || ((uintptr_t)d_out & 15))
        return TOYNI_E_RANGE;
    for (size_t t = 0; t < nslots; ++t)
        if (slots[t].column >= width || slots[t].rotation >= (N >> log_blowup) || slots[t].alpha_index >= (1u << 20) || slots[t].value_index >= (1u << 20))
            return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (nslots == 0) return accumulate ? TOYNI_OK : (int)hipMemsetAsync(d_out, 0, N * 4 * sizeof(uint32_t), s);
    // the slots in the order of the table the kernel reads: sorted by (column, rotation), which does not depend on z
    std::vector<DeepExtSlot> sorted(nslots);
    for (size_t t = 0; t < nslots; ++t)
        sorted[t] = DeepExtSlot{slots[t].column, (uint32_t)((uint64_t)slots[t].rotation << log_blowup), slots[t].alpha_index, slots[t].value_index};
    std::stable_sort(sorted.begin(), sorted.end(), [](const DeepExtSlot& x, const DeepExtSlot& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
    DeepExtArgs a{};
    a.values = d_values;
    a.out = d_out;
    a.col_stride = col_stride;
    a.dom = domain_args(c, (unsigned)log_N, shift);
    a.log_N = (uint32_t)log_N;
    a.nterms = (uint32_t)nslots;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.accumulate = accumulate ? 1u : 0u;
    // the stream's buffer: the record, the table the preparation kernel fills, and (a long table only) the slots it reads
    const bool inline_slots = nslots <= DEEP_EXT_INLINE_SLOTS;
    const size_t table_words = (sizeof(DeepExtRecord) + nslots * sizeof(DeepExtTerm)) / sizeof(uint32_t);
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, table_words + (inline_slots ? 0 : nslots * (sizeof(DeepExtSlot) / sizeof(uint32_t))),
                  sizeof(uint32_t));
    if (rc) return rc;
    DeepExtRecord* rec = reinterpret_cast<DeepExtRecord*>(sc.d_lde32);
    if (inline_slots) {   // capturable: nothing but two launches
        DeepExtInlineSlots in{};
        std::copy(sorted.begin(), sorted.end(), in.s);
        hipLaunchKernelGGL(deep_ext_prepare_inline_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, in, (uint32_t)nslots, d_z, d_alphas, d_claims, rec);
    } else {              // pinned staging ring -> the stream's buffer by a stream-ordered copy, as toyni_deep_combine_ext_device
        DeepExtSlot* d_slots = reinterpret_cast<DeepExtSlot*>(sc.d_lde32 + table_words);
        void* h = nullptr;
        if ((rc = ring_slice(sc, s, nslots * sizeof(DeepExtSlot), &h))) return rc;
        std::memcpy(h, sorted.data(), nslots * sizeof(DeepExtSlot));
        HIPCHK(hipMemcpyAsync(d_slots, h, nslots * sizeof(DeepExtSlot), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(deep_ext_prepare_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, static_cast<const DeepExtSlot*>(d_slots), (uint32_t)nslots, d_z,
                           d_alphas, d_claims, rec);
    }
    const uint64_t items = log_N >= 2 ? N / 4 : N;
    hipLaunchKernelGGL(deep_combine_ext_dz_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a, static_cast<const DeepExtRecord*>(rec));
    return (int)hipGetLastError();
}

// ---- section 3q: the base-field first half of a Fibonacci proof with z in device memory ----
int toyni_mask_poly_device(uint32_t* d_coeffs, size_t n, unsigned mask_degree, const uint8_t key[32], uint64_t nonce, void* stream) {
    if (!d_coeffs || !key) return TOYNI_E_NULL;
    if (mask_degree == 0 || mask_degree > FIB_MASK_MAX_DEGREE || n == 0 || ((uintptr_t)d_coeffs & 3)) return TOYNI_E_RANGE;
    FibMaskArgs a{};
    a.coeffs = d_coeffs;
    a.n = n;
    a.mask_degree = mask_degree;
    std::memcpy(a.key, key, 32);
    a.nonce[0] = 0u;
    a.nonce[1] = (uint32_t)nonce;
    a.nonce[2] = (uint32_t)(nonce >> 32);
    const uint64_t items = fib_mask_items(n, mask_degree);   // <= 2 x 4096: the grid is never capped
    hipLaunchKernelGGL(fib_mask_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int toyni_transcript_squeeze_point_device(toyni_transcript* d_tr, unsigned log_N, uint32_t shift, uint32_t* d_z, void* stream) {
    if (!d_tr || !d_z) return TOYNI_E_NULL;
    if (((uintptr_t)d_tr & 15) || ((uintptr_t)d_z & 3) || log_N > FIB_POINT_MAX_LOG_N || shift == 0 || shift >= BB_P) return TOYNI_E_RANGE;
    hipLaunchKernelGGL(transcript_squeeze_point_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, (hipStream_t)stream, transcript_of(d_tr), (uint32_t)log_N,
                       to_mont_host(bb_inv_host(shift)), d_z);
    return (int)hipGetLastError();
}

int toyni_poly_eval_dz_device(toyni_ntt_ctx* c, const uint32_t* d_coeffs, size_t ncoeffs, const uint32_t* d_z, const uint32_t* mults, unsigned npoints,
                              uint32_t* d_out, void* stream) {
    if (!c || !d_z || !mults || !d_out || (!d_coeffs && ncoeffs)) return TOYNI_E_NULL;
    if (npoints < 1 || npoints > (unsigned)POLY_MAX_POINTS) return TOYNI_E_RANGE;
    PolyDzMults m{};
    for (unsigned p = 0; p < npoints; ++p) {
        if (mults[p] >= BB_P) return TOYNI_E_RANGE;
        m.v[p] = mults[p];
    }
    if (((uintptr_t)d_coeffs | (uintptr_t)d_out | (uintptr_t)d_z) & 3) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (ncoeffs == 0) return (int)hipMemsetAsync(d_out, 0, npoints * sizeof(uint32_t), s);   // the zero polynomial
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    PolyEvalDzArgs a{};
    a.coeffs = d_coeffs;
    a.ncoeffs = ncoeffs;
    a.npoints = npoints;
    a.nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    // the stream's buffer: the partial sums, rounded up to a multiple of four words, then the record
    const size_t partial_words = ((size_t)a.nblocks * npoints + 3) & ~(size_t)3;
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, partial_words + sizeof(PolyDzRecord) / sizeof(uint32_t), sizeof(uint32_t));
    if (rc) return rc;
    a.partial = sc.d_lde32;
    a.out = d_out;
    PolyDzRecord* rec = reinterpret_cast<PolyDzRecord*>(sc.d_lde32 + partial_words);
    hipLaunchKernelGGL(poly_dz_prepare_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, d_z, m, (uint32_t)npoints, rec);
    hipLaunchKernelGGL(poly_eval_partial_dz_kernel, dim3(a.nblocks), dim3(POLY_THREADS), 0, s, a, static_cast<const PolyDzRecord*>(rec));
    hipLaunchKernelGGL(poly_eval_final_dz_kernel, dim3(1), dim3(256), 0, s, a, static_cast<const PolyDzRecord*>(rec));
    return (int)hipGetLastError();
}

int toyni_fib_deep_dz_device(toyni_ntt_ctx* c, const uint32_t* d_trace_lde, const uint32_t* d_q_evals, uint32_t* d_out, unsigned log_blowup,
                             uint32_t shift, const uint32_t* d_z, const uint32_t* d_ood, uint32_t trace_len, uint32_t* d_check, void* stream) {
    if (!c || !d_trace_lde || !d_q_evals || !d_out || !d_z || !d_ood) return TOYNI_E_NULL;
    // decided on the arguments alone, before the context is read
    if (shift == 0 || shift >= BB_P || !is_pow2(trace_len) || trace_len > (1u << 27) || (((uintptr_t)d_z | (uintptr_t)d_ood | (uintptr_t)d_check) & 3))
        return TOYNI_E_RANGE;
    const int log_N = c->plan.log_n;
    if ((int)log_blowup > log_N) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    DeepArgs a{};
    a.trace = d_trace_lde;
    a.quot = d_q_evals;
    a.out = d_out;
    a.dom = domain_args(c, (unsigned)log_N, shift);
    a.log_N = (uint32_t)log_N;
    a.log_blowup = log_blowup;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    FibCheckArgs k{};
    k.log_n = (uint32_t)ilog2(trace_len);
    const uint32_t g_inv = bb_inv_host(bb_root_of_unity_host(k.log_n));   // g^(n-1) = g^-1, g^(n-2) = g^-2
    k.b1R = to_mont_host(g_inv);
    k.b2R = to_mont_host(bb_mul_host(g_inv, g_inv));
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, sizeof(FibDeepRecord) / sizeof(uint32_t), sizeof(uint32_t));
    if (rc) return rc;
    FibDeepRecord* rec = reinterpret_cast<FibDeepRecord*>(sc.d_lde32);
    hipLaunchKernelGGL(fib_deep_prepare_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, d_z, d_ood, k, rec, d_check);
    const uint64_t items = log_N >= 3 ? (1ull << log_N) / 8 : (1ull << log_N);
    hipLaunchKernelGGL(fib_deep_dz_kernel, dim3(grid_for(items)), dim3(256), 0, s, a, static_cast<const FibDeepRecord*>(rec));
    return (int)hipGetLastError();
}

int toyni_fri_phase_roots_device(const uint8_t* d_levels, size_t m_first, unsigned rounds, uint8_t* d_roots, void* stream) {
    if (!d_levels || !d_roots) return TOYNI_E_NULL;
    if (!is_pow2(m_first) || (uint64_t)m_first > ((uint64_t)1 << 32)) return TOYNI_E_INVALID_SIZE;
    if (rounds > FRI_PHASE_MAX_ROUNDS || (rounds && (m_first >> (rounds - 1)) == 0) || ((uintptr_t)d_levels & 15) || ((uintptr_t)d_roots & 3)) return TOYNI_E_RANGE;
    if (rounds == 0) return TOYNI_OK;
    hipLaunchKernelGGL(fri_phase_roots_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const uint32_t*>(d_levels), (uint64_t)m_first,
                       (uint32_t)rounds, reinterpret_cast<uint32_t*>(d_roots));
    return (int)hipGetLastError();
}

// ---- section 3s lives in a translation unit of its own (toyni_hip_fib_batch.hip): what it needs of this one ----
// Not part of the C ABI.  The other unit reads a context through these, and files its launches in this unit's registry.
extern "C++" {   // (this part of the file is inside extern "C")
namespace toyni_internal {
int ctx_log_n(const toyni_ntt_ctx* c) { return c->plan.log_n; }
DomainArgs ctx_domain_args(toyni_ntt_ctx* c, unsigned log_m, uint32_t shift) { return domain_args(c, log_m, shift); }
bool note_launch(const void* kernel) { return launch_registry::note(kernel); }
// enqueue(user, d_words) with the context locked and its device current; words > 0: d_words is the stream's buffer, grown to `words`
int ctx_enqueue(toyni_ntt_ctx* c, void* stream, size_t words, int (*enqueue)(void* user, uint32_t* d_words), void* user) {
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    if (words == 0) return enqueue(user, nullptr);
    hipStream_t s = (hipStream_t)stream;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    if (int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, words, sizeof(uint32_t))) return rc;
    return enqueue(user, sc.d_lde32);
}
}  // namespace toyni_internal
}  // extern "C++"

// ---- section 3g: accumulator columns ----
size_t toyni_column_scan_tile(void) { return SCAN_TILE; }

int toyni_batch_inverse_device(const uint32_t* d_in, uint32_t* d_out, size_t count, uint32_t* d_zero_count, void* stream) {
    if (!d_in || !d_out) return TOYNI_E_NULL;
    if (count > ((size_t)1 << 32) || (((uintptr_t)d_in | (uintptr_t)d_out | (uintptr_t)d_zero_count) & 3)) return TOYNI_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    if (d_zero_count) HIPCHK(hipMemsetAsync(d_zero_count, 0, sizeof(uint32_t), s));
    if (count == 0) return TOYNI_OK;
    hipLaunchKernelGGL(batch_inverse_kernel, dim3((unsigned)((count + SCAN_TILE - 1) / SCAN_TILE)), dim3(SCAN_THREADS), 0, s, d_in, d_out,
                       (uint64_t)count, d_zero_count);
    return (int)hipGetLastError();
}

int toyni_column_scan_device(toyni_ntt_ctx* c, const uint32_t* d_num, size_t num_stride, const uint32_t* d_den, size_t den_stride, uint32_t* d_out,
                             size_t out_stride, size_t n, size_t batch, int op, const uint32_t* init, uint32_t* d_totals, void* stream) {
    // every refusal is decided on the arguments alone: the context is not touched before they have passed
    if (!c || !d_out || !init || (!d_num && !d_den)) return TOYNI_E_NULL;
    if ((op != TOYNI_SCAN_SUM && op != TOYNI_SCAN_PRODUCT) || n > ((size_t)1 << SCAN_MAX_LOG_N) || batch >= ((size_t)1 << 16) ||
        (((uintptr_t)d_num | (uintptr_t)d_den | (uintptr_t)d_out | (uintptr_t)d_totals) & 3))
        return TOYNI_E_RANGE;
    if (batch > 1 && ((d_num && num_stride < n) || (d_den && den_stride < n) || out_stride < n)) return TOYNI_E_RANGE;
    for (size_t b = 0; b < batch; ++b)
        if (init[b] >= BB_P) return TOYNI_E_RANGE;
    if (batch == 0 || n == 0) return TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    ScanArgs a{};
    a.num_stride = num_stride;
    a.den_stride = den_stride;
    a.out_stride = out_stride;
    a.n = n;
    a.ntiles = (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE);
    a.single = a.ntiles == 1 ? 1u : 0u;
    if (!a.single) {   // the aggregates and zero counts of one launch sequence's columns; a warm context finds the buffer in place
        toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
        int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, 2 * (size_t)a.ntiles * std::min<size_t>(batch, SCAN_INLINE_COLUMNS), sizeof(uint32_t));
        if (rc) return rc;
        a.tiles = sc.d_lde32;
    }
    // the seeds ride in the kernel arguments, SCAN_INLINE_COLUMNS columns to a launch sequence (the stream orders the sequences, so
    // they share the buffer)
    for (size_t b0 = 0; b0 < batch; b0 += SCAN_INLINE_COLUMNS) {
        const unsigned cols = (unsigned)std::min<size_t>(batch - b0, SCAN_INLINE_COLUMNS);
        ScanInit in{};
        for (unsigned b = 0; b < cols; ++b) in.v[b] = op == TOYNI_SCAN_PRODUCT ? to_mont_host(init[b0 + b]) : init[b0 + b];
        a.num = d_num ? d_num + b0 * num_stride : nullptr;
        a.den = d_den ? d_den + b0 * den_stride : nullptr;
        a.out = d_out + b0 * out_stride;
        a.totals = d_totals ? d_totals + 2 * b0 : nullptr;
        if (op == TOYNI_SCAN_PRODUCT) column_scan_launch<SCAN_PRODUCT>(a, in, cols, s);
        else column_scan_launch<SCAN_SUM>(a, in, cols, s);
    }
    return (int)hipGetLastError();
}

// ---- section 3i: accumulator columns under an Ext challenge ----
size_t toyni_column_scan_ext_tile(void) { return EXT_ACCUM_TILE; }

int toyni_batch_inverse_ext_device(const uint32_t* d_in, size_t in_stride, uint32_t* d_out, size_t out_stride, size_t count,
                                   uint32_t* d_zero_count, void* stream) {
    if (!d_in || !d_out) return TOYNI_E_NULL;
    if (count > ((size_t)1 << 32) || in_stride < count || out_stride < count ||
        (((uintptr_t)d_in | (uintptr_t)d_out | (uintptr_t)d_zero_count) & 3))
        return TOYNI_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    if (d_zero_count) HIPCHK(hipMemsetAsync(d_zero_count, 0, sizeof(uint32_t), s));
    if (count == 0) return TOYNI_OK;
    hipLaunchKernelGGL(ext_invert_columns_kernel, dim3((unsigned)((count + EXT_ACCUM_TILE - 1) / EXT_ACCUM_TILE)), dim3(EXT_ACCUM_THREADS), 0, s,
                       d_in, (uint64_t)in_stride, d_out, (uint64_t)out_stride, (uint64_t)count, d_zero_count);
    return (int)hipGetLastError();
}

namespace {
// an operand as the header reads it: width 0 or a null pointer is the constant 1.  false: refused.
bool ext_operand_ok(const toyni_ext_operand* o, size_t n, size_t batch, ExtAccumOperand* out) {
    *out = ExtAccumOperand{};
    if (!o || o->width == 0) return true;
    if ((o->width != 1 && o->width != 4) || !o->d_values || ((uintptr_t)o->d_values & 3)) return false;
    if ((o->width == 4 || batch > 1) && o->stride < n) return false;
    for (int k = 0; k < 4; ++k)
        if (o->shift[k] >= BB_P) return false;
    out->values = o->d_values;
    out->stride = o->stride;
    out->width = o->width;
    for (int k = 0; k < 4; ++k) out->shift[k] = o->shift[k];
    return true;
}
}  // namespace

int toyni_column_scan_ext_device(toyni_ntt_ctx* c, const toyni_ext_operand* num, const toyni_ext_operand* den, uint32_t* d_out, size_t out_stride,
                                 size_t n, size_t batch, int op, const uint32_t* init, uint32_t* d_totals, void* stream) {
    // every refusal is decided on the arguments alone: the context is not touched before they have passed
    if (!c || !d_out || !init) return TOYNI_E_NULL;
    ExtAccumArgs a{};
    if (!ext_operand_ok(num, n, batch, &a.num) || !ext_operand_ok(den, n, batch, &a.den) || (a.num.width == 0 && a.den.width == 0)) return TOYNI_E_RANGE;
    if ((op != TOYNI_SCAN_SUM && op != TOYNI_SCAN_PRODUCT) || n > ((size_t)1 << SCAN_MAX_LOG_N) || batch >= ((size_t)1 << 14) || out_stride < n ||
        (((uintptr_t)d_out | (uintptr_t)d_totals) & 3))
        return TOYNI_E_RANGE;
    for (size_t w = 0; w < 4 * batch; ++w)
        if (init[w] >= BB_P) return TOYNI_E_RANGE;
    if (batch == 0 || n == 0) return TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    if (a.den.width == 1) {   // 1 / (shift + v) = 1 / (v - z) with z = -shift: adj_z and m_z, expanded once per call
        uint32_t z[4];
        for (int k = 0; k < 4; ++k) z[k] = a.den.shift[k] ? BB_P - a.den.shift[k] : 0u;
        a.den_inv = ext_shift_host(z);
    }
    a.out_stride = out_stride;
    a.n = n;
    a.ntiles = (uint32_t)((n + EXT_ACCUM_TILE - 1) / EXT_ACCUM_TILE);
    a.single = a.ntiles == 1 ? 1u : 0u;
    if (!a.single) {   // the aggregates and zero counts of one launch sequence's columns; a warm context finds the buffer in place
        toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
        int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words,
                      (size_t)EXT_ACCUM_TILE_WORDS * a.ntiles * std::min<size_t>(batch, EXT_ACCUM_INLINE_COLUMNS), sizeof(uint32_t));
        if (rc) return rc;
        a.tiles = sc.d_lde32;
    }
    // the seeds ride in the kernel arguments, EXT_ACCUM_INLINE_COLUMNS columns to a launch sequence (the stream orders the sequences,
    // so they share the buffer)
    const ExtAccumOperand num0 = a.num, den0 = a.den;
    for (size_t b0 = 0; b0 < batch; b0 += EXT_ACCUM_INLINE_COLUMNS) {
        const unsigned cols = (unsigned)std::min<size_t>(batch - b0, EXT_ACCUM_INLINE_COLUMNS);
        ExtAccumSeeds in{};
        for (unsigned b = 0; b < cols; ++b)
            for (int k = 0; k < 4; ++k) in.v[b][k] = op == TOYNI_SCAN_PRODUCT ? to_mont_host(init[4 * (b0 + b) + k]) : init[4 * (b0 + b) + k];
        a.num.values = num0.values ? num0.values + b0 * num0.width * num0.stride : nullptr;
        a.den.values = den0.values ? den0.values + b0 * den0.width * den0.stride : nullptr;
        a.out = d_out + 4 * b0 * out_stride;
        a.totals = d_totals ? d_totals + 8 * b0 : nullptr;
        if (op == TOYNI_SCAN_PRODUCT) ext_accum_launch<SCAN_PRODUCT>(a, in, cols, s);
        else ext_accum_launch<SCAN_SUM>(a, in, cols, s);
    }
    return (int)hipGetLastError();
}

// ---- section 3f: constraint programs ----
struct toyni_air_program {
    int device = 0;
    toyni_air_info info{};
    AirInsn* d_insns = nullptr;
    uint32_t nparams = 0;    // highest PARAM index + 1 (3p); 0: the program runs under every quotient call
};

// nparams: null for the instruction set of 3f (PARAM is an unknown op); otherwise PARAM is accepted and its highest index + 1 returned
static int air_program_check_impl(const toyni_air_insn* insns, size_t ninsns, toyni_air_info* info, uint32_t* nparams) {
    if (!insns || !info) return TOYNI_E_NULL;
    if (ninsns == 0 || ninsns > AIR_MAX_INSNS) return TOYNI_E_RANGE;
    toyni_air_info r{};
    r.ninsns = (uint32_t)ninsns;
    bool written[AIR_MAX_REGS] = {};
    bool emitted = false;
    uint32_t np = 0;
    const auto readable = [&](uint8_t reg) { return reg < AIR_MAX_REGS && written[reg]; };
    for (size_t k = 0; k < ninsns; ++k) {
        const toyni_air_insn& in = insns[k];
        if (in.op >= AIR_OP_COUNT && !(nparams && in.op == TOYNI_AIR_PARAM)) return TOYNI_E_RANGE;
        if (in.op == TOYNI_AIR_EMIT) {
            if (!readable(in.a) || in.b > 1 || in.imm >= 65536) return TOYNI_E_RANGE;
            r.nconstraints = std::max(r.nconstraints, in.imm + 1);
            if (in.b == 0) r.divides_by_zh = 1;
            emitted = true;
            continue;
        }
        if (in.dst >= AIR_MAX_REGS) return TOYNI_E_RANGE;
        if (in.op == TOYNI_AIR_PARAM) {
            if (in.imm >= AIR_MAX_PARAMS) return TOYNI_E_RANGE;
            np = std::max(np, in.imm + 1);
        } else if (in.op >= TOYNI_AIR_ADD) {
            if (!readable(in.a) || !readable(in.b)) return TOYNI_E_RANGE;
        } else if (in.op == TOYNI_AIR_CELL) {
            if (in.b >= AIR_MAX_MATRICES || in.imm >= 65536) return TOYNI_E_RANGE;
            r.nmatrices = std::max<uint32_t>(r.nmatrices, in.b + 1u);
            r.min_width[in.b] = std::max(r.min_width[in.b], in.imm + 1);
            r.max_rotation = std::max<uint32_t>(r.max_rotation, in.a);
        } else if (in.op != TOYNI_AIR_X && in.imm >= BB_P) {   // CONST, XINV
            return TOYNI_E_RANGE;
        }
        written[in.dst] = true;
    }
    if (!emitted) return TOYNI_E_RANGE;
    for (uint32_t k = 0; k < AIR_MAX_REGS; ++k)
        if (written[k]) r.nregs = k + 1;   // a register that is read has been written
    *info = r;
    if (nparams) *nparams = np;
    return TOYNI_OK;
}
int toyni_air_program_check(const toyni_air_insn* insns, size_t ninsns, toyni_air_info* info) {
    return air_program_check_impl(insns, ninsns, info, nullptr);
}
int toyni_air_program_check_params(const toyni_air_insn* insns, size_t ninsns, toyni_air_info* info, uint32_t* nparams) {
    if (!nparams) return TOYNI_E_NULL;
    return air_program_check_impl(insns, ninsns, info, nparams);
}

static int air_program_create_impl(toyni_ntt_ctx* c, const toyni_air_insn* insns, size_t ninsns, toyni_air_program** out, bool with_params) {
    if (!c || !insns || !out) return TOYNI_E_NULL;
    toyni_air_info info{};
    uint32_t nparams = 0;
    if (int rc = air_program_check_impl(insns, ninsns, &info, with_params ? &nparams : nullptr)) return rc;
    std::vector<AirInsn> dev(ninsns);
    for (size_t k = 0; k < ninsns; ++k) {
        const toyni_air_insn& in = insns[k];
        dev[k].w0 = (uint32_t)in.op | (uint32_t)in.dst << 8 | (uint32_t)in.a << 16 | (uint32_t)in.b << 24;
        dev[k].imm = (in.op == TOYNI_AIR_CONST || in.op == TOYNI_AIR_XINV) ? to_mont_host(in.imm) : in.imm;
    }
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    toyni_air_program* p = new toyni_air_program();
    p->device = c->device;
    p->info = info;
    p->nparams = nparams;
    hipError_t e = hipMalloc((void**)&p->d_insns, ninsns * sizeof(AirInsn));
    if (e == hipSuccess) e = hipMemcpy(p->d_insns, dev.data(), ninsns * sizeof(AirInsn), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (p->d_insns) (void)hipFree(p->d_insns);
        delete p;
        return (int)e;
    }
    *out = p;
    return TOYNI_OK;
}
int toyni_air_program_create(toyni_ntt_ctx* c, const toyni_air_insn* insns, size_t ninsns, toyni_air_program** out) {
    return air_program_create_impl(c, insns, ninsns, out, false);
}
int toyni_air_program_create_params(toyni_ntt_ctx* c, const toyni_air_insn* insns, size_t ninsns, toyni_air_program** out) {
    return air_program_create_impl(c, insns, ninsns, out, true);
}
int toyni_air_program_nparams(const toyni_air_program* p, uint32_t* nparams) {
    if (!p || !nparams) return TOYNI_E_NULL;
    *nparams = p->nparams;
    return TOYNI_OK;
}

int toyni_air_program_destroy(toyni_air_program* p) {
    if (!p) return TOYNI_OK;
    DeviceGuard guard(p->device);
    (void)hipDeviceSynchronize();   // a call in flight may still read the program
    const hipError_t e = hipFree(p->d_insns);
    delete p;
    return (int)e;
}

int toyni_air_program_info(const toyni_air_program* p, toyni_air_info* info) {
    if (!p || !info) return TOYNI_E_NULL;
    *info = p->info;
    return TOYNI_OK;
}

// What both quotient entries (3f, 3k) refuse on the program, the matrices, the coset and the pointers, in 3f's order; the weights'
// values are the caller's to check next, Z_H after them (air_quotient_args)
static int air_quotient_check(const toyni_ntt_ctx* c, const toyni_air_program* prog, const toyni_air_matrix* mats, size_t nmats, unsigned log_blowup,
                              uint32_t shift, size_t nweights, const uint32_t* d_c_out, const uint32_t* d_q_out) {
    const toyni_air_info& info = prog->info;
    const int log_N = c->plan.log_n;
    const uint64_t N = 1ull << log_N;
    if (prog->device != c->device || nmats < info.nmatrices || nmats > AIR_MAX_MATRICES || (int)log_blowup > log_N || shift == 0 || shift >= BB_P ||
        nweights < info.nconstraints || nweights > 65536 || (((uintptr_t)d_c_out | (uintptr_t)d_q_out) & 3))
        return TOYNI_E_RANGE;
    if (info.max_rotation >= (N >> log_blowup)) return TOYNI_E_RANGE;
    for (uint32_t m = 0; m < info.nmatrices; ++m)
        if (info.min_width[m] && (!mats[m].d_values || ((uintptr_t)mats[m].d_values & 3) || mats[m].width < info.min_width[m] || mats[m].width > 65536 ||
                                  mats[m].col_stride < N))
            return TOYNI_E_RANGE;
    return TOYNI_OK;
}
// the kernel arguments and the launch shape of a call that passed air_quotient_check; TOYNI_E_ZERO_INVERSE where Z_H vanishes on the coset
static int air_quotient_args(toyni_ntt_ctx* c, const toyni_air_program* prog, const toyni_air_matrix* mats, unsigned log_blowup, uint32_t shift,
                             uint32_t* d_c_out, uint32_t* d_q_out, int accumulate, AirArgs& a, AirLaunchShape& shape, dim3& grid) {
    const toyni_air_info& info = prog->info;
    const int log_N = c->plan.log_n;
    const uint64_t N = 1ull << log_N;
    const uint64_t n = N >> log_blowup;
    const uint32_t shift_n = bb_pow_host(shift, n);
    // Z_H(x) = 0 on the coset only if shift^n is a B-th root of unity (toyni_fib_quotient_device)
    if (info.divides_by_zh && bb_pow_host(shift_n, 1ull << log_blowup) == 1u) return TOYNI_E_ZERO_INVERSE;
    a = AirArgs{};
    a.insns = prog->d_insns;
    for (uint32_t m = 0; m < info.nmatrices; ++m) {
        a.mat[m] = info.min_width[m] ? mats[m].d_values : nullptr;
        a.col_stride[m] = mats[m].col_stride;
    }
    a.c_out = d_c_out;
    a.q_out = d_q_out;
    a.dom = domain_args(c, (unsigned)log_N, shift);
    a.ninsns = info.ninsns;
    a.nregs = info.nregs;
    a.log_N = (uint32_t)log_N;
    a.log_blowup = log_blowup;
    a.wNR = to_mont_host(bb_root_of_unity_host((uint32_t)log_N));
    a.shift_nR = to_mont_host(shift_n);
    a.wBR = to_mont_host(bb_pow_host(bb_root_of_unity_host((uint32_t)log_N), n));
    a.divides = info.divides_by_zh;
    a.accumulate = accumulate ? 1u : 0u;
    shape = air_launch_shape(info.nregs, info.divides_by_zh, log_blowup);   // prover_kernels.hpp
    a.zh_lds = shape.zh_lds;
    const uint64_t items = log_N >= 2 ? N / 4 : N;
    grid = dim3((unsigned)((items + shape.threads - 1) / shape.threads));
    return TOYNI_OK;
}

int toyni_air_quotient_device(toyni_ntt_ctx* c, const toyni_air_program* prog, const toyni_air_matrix* mats, size_t nmats, unsigned log_blowup,
                              uint32_t shift, const uint32_t* weights, size_t nweights, uint32_t* d_c_out, uint32_t* d_q_out, int accumulate,
                              void* stream) {
    if (!c || !prog || !weights || !d_q_out || (!mats && nmats)) return TOYNI_E_NULL;
    if (prog->nparams) return TOYNI_E_RANGE;   // a PARAM needs the parameter array of 3p
    if (int rc = air_quotient_check(c, prog, mats, nmats, log_blowup, shift, nweights, d_c_out, d_q_out)) return rc;
    for (size_t k = 0; k < nweights; ++k)
        if (weights[k] >= BB_P) return TOYNI_E_RANGE;
    AirArgs a;
    AirLaunchShape shape;
    dim3 grid;
    if (int rc = air_quotient_args(c, prog, mats, log_blowup, shift, d_c_out, d_q_out, accumulate, a, shape, grid)) return rc;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    const unsigned threads = shape.threads;
    const size_t lds = shape.lds_bytes;
    if (nweights <= AIR_INLINE_WEIGHTS) {   // the weights ride in the kernel arguments
        AirInlineWeights in{};
        std::copy(weights, weights + nweights, in.w);
        hipLaunchKernelGGL(air_quotient_inline_kernel, grid, dim3(threads), lds, s, a, in);
        return (int)hipGetLastError();
    }
    // more weights: pinned staging ring -> the stream's intermediate buffer by a stream-ordered copy (toyni_deep_combine_device)
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, nweights, sizeof(uint32_t));
    if (rc) return rc;
    void* h = nullptr;
    if ((rc = ring_slice(sc, s, nweights * sizeof(uint32_t), &h))) return rc;
    std::memcpy(h, weights, nweights * sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(sc.d_lde32, h, nweights * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(air_quotient_kernel, grid, dim3(threads), lds, s, a, sc.d_lde32);
    return (int)hipGetLastError();
}

// ---- section 3k: the same programs under Ext weights, one interpretation per point ----
int toyni_air_quotient_ext_device(toyni_ntt_ctx* c, const toyni_air_program* prog, const toyni_air_matrix* mats, size_t nmats, unsigned log_blowup,
                                  uint32_t shift, const uint32_t* weights4, size_t nweights, uint32_t* d_c_out, uint32_t* d_q_out, size_t out_stride,
                                  int accumulate, void* stream) {
    if (!c || !prog || !weights4 || !d_q_out || (!mats && nmats)) return TOYNI_E_NULL;
    if (prog->nparams) return TOYNI_E_RANGE;   // a PARAM needs the parameter array of 3p
    if (int rc = air_quotient_check(c, prog, mats, nmats, log_blowup, shift, nweights, d_c_out, d_q_out)) return rc;
    if (out_stride < ((size_t)1 << c->plan.log_n)) return TOYNI_E_RANGE;
    for (size_t k = 0; k < 4 * nweights; ++k)
        if (weights4[k] >= BB_P) return TOYNI_E_RANGE;
    AirArgs a;
    AirLaunchShape shape;
    dim3 grid;
    if (int rc = air_quotient_args(c, prog, mats, log_blowup, shift, d_c_out, d_q_out, accumulate, a, shape, grid)) return rc;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t stride = out_stride;
    if (nweights <= AIR_EXT_INLINE_WEIGHTS) {   // the weights ride in the kernel arguments
        AirExtInlineWeights in{};
        std::copy(weights4, weights4 + 4 * nweights, in.w);
        hipLaunchKernelGGL(air_quotient_ext_inline_kernel, grid, dim3(shape.threads), (size_t)shape.lds_bytes, s, a, stride, in);
        return (int)hipGetLastError();
    }
    // more weights: pinned staging ring -> the stream's intermediate buffer, as toyni_air_quotient_device
    const size_t words = 4 * nweights;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, words, sizeof(uint32_t));
    if (rc) return rc;
    void* h = nullptr;
    if ((rc = ring_slice(sc, s, words * sizeof(uint32_t), &h))) return rc;
    std::memcpy(h, weights4, words * sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(sc.d_lde32, h, words * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(air_quotient_ext_kernel, grid, dim3(shape.threads), (size_t)shape.lds_bytes, s, a, stride, (const uint32_t*)sc.d_lde32);
    return (int)hipGetLastError();
}

// ---- section 3p: gamma and the constraint weights in device memory ----
int toyni_air_quotient_ext_dc_device(toyni_ntt_ctx* c, const toyni_air_program* prog, const toyni_air_matrix* mats, size_t nmats, unsigned log_blowup,
                                     uint32_t shift, const uint32_t* d_params, size_t nparams, const uint32_t* d_alphas, size_t nalphas,
                                     int weights_form, uint32_t* d_c_out, uint32_t* d_q_out, size_t out_stride, int accumulate, void* stream) {
    if (!c || !prog || !d_alphas || !d_q_out || (!mats && nmats) || (!d_params && nparams)) return TOYNI_E_NULL;
    if (weights_form != TOYNI_AIR_WEIGHTS_EXT && weights_form != TOYNI_AIR_WEIGHTS_EMIT_EXT) return TOYNI_E_RANGE;
    // (decided on the arguments alone, before the program or the context is read)
    if (nparams > AIR_MAX_PARAMS || nalphas > AIR_DC_MAX_WEIGHTS || (((uintptr_t)d_params | (uintptr_t)d_alphas) & 3)) return TOYNI_E_RANGE;
    if (nparams < prog->nparams) return TOYNI_E_RANGE;
    const size_t nweights = air_dc_nweights((uint32_t)nalphas, (uint32_t)weights_form);
    if (int rc = air_quotient_check(c, prog, mats, nmats, log_blowup, shift, nweights, d_c_out, d_q_out)) return rc;
    if (out_stride < ((size_t)1 << c->plan.log_n)) return TOYNI_E_RANGE;
    AirArgs a;
    AirLaunchShape shape;
    dim3 grid;
    if (int rc = air_quotient_args(c, prog, mats, log_blowup, shift, d_c_out, d_q_out, accumulate, a, shape, grid)) return rc;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    // the stream's buffer holds the record; both launches are ordered by the stream, so the call is a chain of two kernels
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, air_dc_record_words((uint32_t)nparams, (uint32_t)nalphas, (uint32_t)weights_form),
                  sizeof(uint32_t));
    if (rc) return rc;
    uint32_t* rec = sc.d_lde32;
    hipLaunchKernelGGL(air_dc_prepare_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, d_params, (uint32_t)nparams, d_alphas, (uint32_t)nalphas,
                       (uint32_t)weights_form, rec);
    hipLaunchKernelGGL(air_quotient_ext_dc_kernel, grid, dim3(shape.threads), (size_t)shape.lds_bytes, s, a, (uint64_t)out_stride,
                       static_cast<const uint32_t*>(rec), (uint32_t)nparams);
    return (int)hipGetLastError();
}

namespace {
// ext_operand_ok for an operand whose shift is an index into the challenges; *index: what the preparation kernel reads
bool ext_operand_dc_ok(const toyni_ext_operand_dc* o, size_t n, size_t batch, ExtAccumOperand* out, uint32_t* index) {
    *out = ExtAccumOperand{};
    *index = EXT_SHIFT_NONE;
    if (!o || o->width == 0) return true;
    if ((o->width != 1 && o->width != 4) || !o->d_values || ((uintptr_t)o->d_values & 3)) return false;
    if ((o->width == 4 || batch > 1) && o->stride < n) return false;
    if (o->shift_index != TOYNI_EXT_SHIFT_NONE && o->shift_index >= EXT_SHIFT_MAX_INDEX) return false;
    out->values = o->d_values;
    out->stride = o->stride;
    out->width = o->width;
    *index = o->shift_index;
    return true;
}
}  // namespace

int toyni_column_scan_ext_dc_device(toyni_ntt_ctx* c, const toyni_ext_operand_dc* num, const toyni_ext_operand_dc* den, const uint32_t* d_challenges,
                                    uint32_t* d_out, size_t out_stride, size_t n, size_t batch, int op, const uint32_t* init, uint32_t* d_totals,
                                    void* stream) {
    // every refusal is decided on the arguments alone: the context is not touched before they have passed
    if (!c || !d_out || !init) return TOYNI_E_NULL;
    ExtAccumArgs a{};
    uint32_t num_index, den_index;
    if (!ext_operand_dc_ok(num, n, batch, &a.num, &num_index) || !ext_operand_dc_ok(den, n, batch, &a.den, &den_index) ||
        (a.num.width == 0 && a.den.width == 0))
        return TOYNI_E_RANGE;
    if ((num_index != EXT_SHIFT_NONE || den_index != EXT_SHIFT_NONE) && !d_challenges) return TOYNI_E_NULL;
    if ((op != TOYNI_SCAN_SUM && op != TOYNI_SCAN_PRODUCT) || n > ((size_t)1 << SCAN_MAX_LOG_N) || batch >= ((size_t)1 << 14) || out_stride < n ||
        (((uintptr_t)d_out | (uintptr_t)d_totals | (uintptr_t)d_challenges) & 3))
        return TOYNI_E_RANGE;
    for (size_t w = 0; w < 4 * batch; ++w)
        if (init[w] >= BB_P) return TOYNI_E_RANGE;
    if (batch == 0 || n == 0) return TOYNI_OK;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    a.out_stride = out_stride;
    a.n = n;
    a.ntiles = (uint32_t)((n + EXT_ACCUM_TILE - 1) / EXT_ACCUM_TILE);
    a.single = a.ntiles == 1 ? 1u : 0u;
    // the stream's buffer: the tile words of one launch sequence's columns (none for a single tile), then the record, 16-byte aligned
    const size_t tile_words = a.single ? 0 : (size_t)EXT_ACCUM_TILE_WORDS * a.ntiles * std::min<size_t>(batch, EXT_ACCUM_INLINE_COLUMNS);
    const size_t rec_at = (tile_words + 3) & ~(size_t)3;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    int rc = grow(c, s, (void**)&sc.d_lde32, &sc.lde32_words, rec_at + sizeof(ExtAccumRecord) / sizeof(uint32_t), sizeof(uint32_t));
    if (rc) return rc;
    a.tiles = a.single ? nullptr : sc.d_lde32;
    ExtAccumRecord* rec = reinterpret_cast<ExtAccumRecord*>(sc.d_lde32 + rec_at);
    hipLaunchKernelGGL(extcol_dc_prepare_kernel, dim3(1), dim3(TRANSCRIPT_T), 0, s, d_challenges, num_index, den_index,
                       a.den.width == 1 ? 1u : 0u, rec);
    // one record serves every launch sequence of the call
    const ExtAccumOperand num0 = a.num, den0 = a.den;
    for (size_t b0 = 0; b0 < batch; b0 += EXT_ACCUM_INLINE_COLUMNS) {
        const unsigned cols = (unsigned)std::min<size_t>(batch - b0, EXT_ACCUM_INLINE_COLUMNS);
        ExtAccumSeeds in{};
        for (unsigned b = 0; b < cols; ++b)
            for (int k = 0; k < 4; ++k) in.v[b][k] = op == TOYNI_SCAN_PRODUCT ? to_mont_host(init[4 * (b0 + b) + k]) : init[4 * (b0 + b) + k];
        a.num.values = num0.values ? num0.values + b0 * num0.width * num0.stride : nullptr;
        a.den.values = den0.values ? den0.values + b0 * den0.width * den0.stride : nullptr;
        a.out = d_out + 4 * b0 * out_stride;
        a.totals = d_totals ? d_totals + 8 * b0 : nullptr;
        if (op == TOYNI_SCAN_PRODUCT) ext_accum_dc_launch<SCAN_PRODUCT>(a, in, static_cast<const ExtAccumRecord*>(rec), cols, s);
        else ext_accum_dc_launch<SCAN_SUM>(a, in, static_cast<const ExtAccumRecord*>(rec), cols, s);
    }
    return (int)hipGetLastError();
}

size_t toyni_merkle_open_record_bytes(size_t n) { return n ? (size_t)merkle_open_record_bytes(n) : 0; }

int toyni_merkle_open_device(const uint8_t* d_levels, size_t n, const uint32_t* d_values, const uint8_t* d_salts, const uint32_t* d_indices,
                             size_t nidx, uint8_t* d_out, void* stream) {
    if (!d_levels || !d_values || !d_indices || !d_out) return TOYNI_E_NULL;
    if (n == 0 || nidx == 0) return TOYNI_OK;
    if (n > 0xFFFFFFFFull || nidx > 0xFFFFFFFFull || ((uintptr_t)d_levels & 15) || ((uintptr_t)d_salts & 15) || ((uintptr_t)d_out & 7)) return TOYNI_E_RANGE;
    const uint64_t work = (uint64_t)nidx * (merkle_depth(n) + 1);
    const OpenGroup g{reinterpret_cast<const Digest*>(d_levels), (uint64_t)n, d_values, reinterpret_cast<const uint4*>(d_salts), d_indices, (uint32_t)nidx, d_out};
    hipLaunchKernelGGL(merkle_open_kernel, dim3(grid_for(work)), dim3(256), 0, (hipStream_t)stream, g);
    return (int)hipGetLastError();
}

// The openings of several trees (a proof's query phase: trace, quotient, DEEP and every FRI layer) gathered by one launch per 32 trees.
int toyni_merkle_open_groups_device(const toyni_merkle_open_group* groups, size_t ngroups, void* stream) {
    if (!groups && ngroups) return TOYNI_E_NULL;
    for (size_t k = 0; k < ngroups; ++k) {
        const toyni_merkle_open_group& q = groups[k];
        if (q.n == 0 || q.nidx == 0) continue;
        if (!q.d_levels || !q.d_values || !q.d_indices || !q.d_out) return TOYNI_E_NULL;
        if (q.n > 0xFFFFFFFFull || q.nidx > 0xFFFFFFFFull || ((uintptr_t)q.d_levels & 15) || ((uintptr_t)q.d_salts & 15) || ((uintptr_t)q.d_out & 7)) return TOYNI_E_RANGE;
    }
    for (size_t k0 = 0; k0 < ngroups; k0 += OPEN_GROUPS_MAX) {
        OpenGroups gs{};
        uint32_t cnt = 0;
        uint64_t most = 0;
        for (size_t k = k0; k < ngroups && k < k0 + OPEN_GROUPS_MAX; ++k) {
            const toyni_merkle_open_group& q = groups[k];
            if (q.n == 0 || q.nidx == 0) continue;
            gs.g[cnt++] = OpenGroup{reinterpret_cast<const Digest*>(q.d_levels), (uint64_t)q.n, q.d_values, reinterpret_cast<const uint4*>(q.d_salts), q.d_indices,
                                    (uint32_t)q.nidx, q.d_out};
            const uint64_t work = (uint64_t)q.nidx * (merkle_depth(q.n) + 1);
            if (work > most) most = work;
        }
        if (!cnt) continue;
        hipLaunchKernelGGL(merkle_open_groups_kernel, dim3(grid_for(most), cnt), dim3(256), 0, (hipStream_t)stream, gs);
        HIPCHK(hipGetLastError());
    }
    return TOYNI_OK;
}

// ---- plumbing ----
int toyni_malloc(void** d_ptr, size_t bytes) { return d_ptr ? (int)hipMalloc(d_ptr, bytes) : TOYNI_E_NULL; }
int toyni_free(void* d_ptr) { return (int)hipFree(d_ptr); }
int toyni_host_alloc(void** h_ptr, size_t bytes) { return h_ptr ? (int)hipHostMalloc(h_ptr, bytes, hipHostMallocPortable) : TOYNI_E_NULL; }
int toyni_host_free(void* h_ptr) { return (int)hipHostFree(h_ptr); }
int toyni_memcpy_h2d(void* d, const void* h, size_t bytes) { return (int)hipMemcpy(d, h, bytes, hipMemcpyHostToDevice); }
int toyni_memcpy_d2h(void* h, const void* d, size_t bytes) { return (int)hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost); }
// stream-ordered forms: what a device-resident pipeline in a host language without a HIP binding needs between the calls of this
// header (csrc/host/fib_prover.hpp is written against exactly these)
int toyni_memcpy_h2d_async(void* d, const void* h, size_t bytes, void* stream) {
    return bytes ? (int)hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, (hipStream_t)stream) : TOYNI_OK;
}
int toyni_memcpy_d2h_async(void* h, const void* d, size_t bytes, void* stream) {
    return bytes ? (int)hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) : TOYNI_OK;
}
int toyni_memcpy_d2d_async(void* dst, const void* src, size_t bytes, void* stream) {
    return bytes ? (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) : TOYNI_OK;
}
int toyni_memset_async(void* d, int value, size_t bytes, void* stream) {
    return bytes ? (int)hipMemsetAsync(d, value, bytes, (hipStream_t)stream) : TOYNI_OK;
}

int toyni_chacha20_fill_device(void* d_out, size_t bytes, const uint8_t key[32], uint64_t nonce, void* stream) {
    if (!d_out || !key) return TOYNI_E_NULL;
    if (((uintptr_t)d_out & 15) || (bytes & 63)) return TOYNI_E_RANGE;   // whole 64-byte blocks, 16-byte stores
    if (bytes == 0) return TOYNI_OK;
    if (bytes / 64 > 0xFFFFFFFFull) return TOYNI_E_RANGE;               // RFC 8439's 32-bit block counter
    ChaChaArgs a{};
    std::memcpy(a.key, key, 32);
    a.nonce[0] = 0u;
    a.nonce[1] = (uint32_t)nonce;
    a.nonce[2] = (uint32_t)(nonce >> 32);
    a.blocks = bytes / 64;
    a.out = reinterpret_cast<uint4*>(d_out);
    hipLaunchKernelGGL(chacha20_fill_kernel, dim3(grid_for(a.blocks)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int toyni_narrow_u64_to_u32(const uint64_t* d_in, uint32_t* d_out, size_t count, void* stream) {
    if (!d_in || !d_out) return TOYNI_E_NULL;
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 3)) return TOYNI_E_RANGE;
    if (!count) return TOYNI_OK;
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, d_in, d_out, count);
    return (int)hipGetLastError();
}

int toyni_widen_u32_to_u64(const uint32_t* d_in, uint64_t* d_out, size_t count, void* stream) {
    if (!d_in || !d_out) return TOYNI_E_NULL;
    if (((uintptr_t)d_in & 3) || ((uintptr_t)d_out & 7)) return TOYNI_E_RANGE;
    if (!count) return TOYNI_OK;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for(count)), dim3(256), 0, (hipStream_t)stream, d_in, d_out, count);
    return (int)hipGetLastError();
}

// Streams for callers without a HIP binding of their own (the Rust crate binds this library only): every `stream` argument of
// this header is a hipStream_t, and these two make and release one (non-blocking with respect to the legacy default stream).
int toyni_stream_create(void** stream, int device) {
    if (!stream) return TOYNI_E_NULL;
    *stream = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); return TOYNI_E_NO_DEVICE; }
    if (device < 0) HIPCHK(hipGetDevice(&device));
    if (device >= count) return TOYNI_E_RANGE;
    DeviceGuard guard(device);
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream = (void*)s;
    return TOYNI_OK;
}

// Waits for the stream's work, then destroys it.  Scratch sets that contexts keep for this stream are released by their
// own fences (see "Threading and streams" in the header); nothing needs to be told about the destruction.
int toyni_stream_destroy(void* stream) {
    if (!stream) return TOYNI_OK;
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return (int)hipStreamDestroy((hipStream_t)stream);
}

// Cross-stream ordering without exposing events: everything enqueued on `stream` after this call waits for everything enqueued on
// `after` before it.  (An event is created, recorded on `after`, waited for on `stream` and released; the wait stays enqueued.)
int toyni_stream_wait(void* stream, void* after) {
    if (stream == after) return TOYNI_OK;
    hipEvent_t ev = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, (hipStream_t)after);
    if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)stream, ev, 0);
    (void)hipEventDestroy(ev);   // released once the recorded work has completed; the enqueued wait keeps its own reference
    return (int)e;
}

// Events (timing disabled): record on one stream now, let another stream wait for that point later.
int toyni_event_create(void** event) {
    if (!event) return TOYNI_E_NULL;
    hipEvent_t ev = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    *event = (void*)ev;
    return TOYNI_OK;
}
int toyni_event_destroy(void* event) { return event ? (int)hipEventDestroy((hipEvent_t)event) : TOYNI_OK; }
int toyni_event_record(void* event, void* stream) { return event ? (int)hipEventRecord((hipEvent_t)event, (hipStream_t)stream) : TOYNI_E_NULL; }
int toyni_stream_wait_event(void* stream, void* event) { return event ? (int)hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0) : TOYNI_E_NULL; }

int toyni_stream_synchronize(toyni_ntt_ctx* c, void* stream) {
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (c) {
        TOYNI_CTX_LOCK(c);
        DeviceGuard guard(c->device);
        reclaim_after_sync(c, (hipStream_t)stream);
    }
    return TOYNI_OK;
}

int toyni_ntt_ctx_trim(toyni_ntt_ctx* c) {
    if (!c) return TOYNI_E_NULL;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    HIPCHK(hipDeviceSynchronize());
    for (auto& kv : c->scratch) { kv.second.dirty = false; retire_scratch(c, kv.second, kv.first, false); }
    c->scratch.clear();
    for (size_t i = 0; i < c->retired.size(); ++i) { (void)hipFree(c->retired[i].ptr); c->retired[i].ptr = nullptr; }
    for (size_t i = 0; i < c->retired.size(); ++i) { drop_retired_event(c, i); c->retired[i].ev = nullptr; }
    c->retired.clear();
    return TOYNI_OK;
}

#ifdef TOYNI_TOOLS  // include/toyni_hip_tools.h
// Times the passes of the PASS PLAN the route names for this batch (the main plan or, at n = 2^21 / 2^22, the two-pass one) -- also
// where the route is a sweep (n = 2^11 .. 2^15 from their thresholds up), whose one kernel this does not time.
int toyni_ntt_profile_passes(toyni_ntt_ctx* c, uint32_t* d_data, size_t batch, int inverse, int reps, float* ms_per_pass, void* stream) {
    if (!c || !d_data || !ms_per_pass) return TOYNI_E_NULL;
    if (reps < 1 || batch < 1) return TOYNI_E_RANGE;
    TOYNI_CTX_LOCK(c);
    DeviceGuard guard(c->device);
    hipStream_t s = (hipStream_t)stream;
    toyni_ntt_ctx::Scratch& sc = scratch_for(c, s);
    if (c->plan.log_n == 0) return TOYNI_OK;
    if (c->plan.npasses > 1) {
        int rc = grow(c, s, (void**)&sc.d_work, &sc.work_words, batch * (size_t)c->n, sizeof(uint32_t));
        if (rc) return rc;
    }
    const bool lat = route_of(c, batch).lat;
    const uint32_t* tables = lat ? (inverse ? c->d_inv_lat : c->d_fwd_lat) : (inverse ? c->d_inv : c->d_fwd);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    int pass_index = 0;
    hipError_t err = hipSuccess;
    bool ok = for_each_pass(launch_knobs(), lat ? c->plan_lat : c->plan, tables, inverse != 0, d_data, sc.d_work, d_data, batch,
                            [&](auto pass, auto, const PassArgs& a, uint64_t nblocks) {
                                using P = decltype(pass);
                                if (err != hipSuccess) return;
                                const unsigned grid = persistent_grid<P>(c, nblocks);
                                launch_pass<P>(grid, s, a, (uint32_t)nblocks);  // warm
                                (void)hipEventRecord(e0, s);
                                for (int r = 0; r < reps; ++r) launch_pass<P>(grid, s, a, (uint32_t)nblocks);
                                (void)hipEventRecord(e1, s);
                                err = hipEventSynchronize(e1);
                                float ms = 0.f;
                                if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
                                ms_per_pass[pass_index++] = ms / (float)reps;
                            });
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (!ok) return TOYNI_E_INVALID_SIZE;
    return (int)err;
}
#endif  // TOYNI_TOOLS

// ---- the reference's ABI, symbol for symbol (include/toyni_hip.h section 1) ----
void* ntt_ctx_create(uint32_t n) {
    toyni_ntt_ctx* c = nullptr;
    return toyni_ntt_ctx_create(n, -1, &c) == TOYNI_OK ? (void*)c : nullptr;  // cuda/ntt_kernel.cu:217-220: nullptr on error
}
void ntt_ctx_destroy(void* ctx) { (void)toyni_ntt_ctx_destroy((toyni_ntt_ctx*)ctx); }
void ntt_run_inplace(void* ctx, uint64_t* h_data) {
    int rc = toyni_ntt_host((toyni_ntt_ctx*)ctx, h_data, 1, 0);
    if (rc) std::fprintf(stderr, "toyni_hip: ntt_run_inplace failed: %s\n", toyni_error_string(rc));  // void ABI: cannot return it
}
void intt_run_inplace(void* ctx, uint64_t* h_data) {
    int rc = toyni_ntt_host((toyni_ntt_ctx*)ctx, h_data, 1, 1);
    if (rc) std::fprintf(stderr, "toyni_hip: intt_run_inplace failed: %s\n", toyni_error_string(rc));
}
int cuda_malloc(uint64_t** d_ptr, size_t count) { return d_ptr ? (int)hipMalloc((void**)d_ptr, count * sizeof(uint64_t)) : TOYNI_E_NULL; }
int cuda_free(uint64_t* d_ptr) { return (int)hipFree(d_ptr); }
int cuda_copy_to_device(uint64_t* d_dest, const uint64_t* h_src, size_t count) {
    return (int)hipMemcpy(d_dest, h_src, count * sizeof(uint64_t), hipMemcpyHostToDevice);
}
int cuda_copy_from_device(uint64_t* h_dest, const uint64_t* d_src, size_t count) {
    return (int)hipMemcpy(h_dest, d_src, count * sizeof(uint64_t), hipMemcpyDeviceToHost);
}
const char* cuda_get_error_string(int error) { return toyni_error_string(error); }

}  // extern "C"

// multi-GPU forms for a single-process host: cached per-device contexts, batch sharding, one transform over G devices
#include "multi_gpu.hpp"
#endif  // TOYNI_KERNEL_TEXT_ONLY
