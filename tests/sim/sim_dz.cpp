// Runs the kernels of include/toyni_hip.h 3o themselves -- poly_ext_prepare_kernel, poly_eval_ext_batch_partial_dz_kernel,
// poly_eval_ext_batch_final_dz_kernel, deep_ext_prepare_inline_kernel, deep_ext_prepare_kernel, deep_combine_ext_dz_kernel,
// transcript_squeeze_ext_point_kernel, transcript_absorb_fields_kernel, query_rows_kernel of toyni_amd/csrc/toyni_hip.hip -- on the
// CPU through hip_sim.hpp (unchanged), every GPU thread a fiber, under the eight wave / lane schedules of that header.
//
// TEST INFRASTRUCTURE (tests/test_sim_dz.py; tests/test_field_contracts_dz.py rebuilds it with tests/emu/field_contracts.hpp in
// front).  The driver arranges the buffers as the entry points do (the partial sums and then the record; the record, the table and
// then the staged slots; the slots sorted by (column, rotation)) and expects nothing itself: it prints the inputs and, for the first
// schedule, every output word; the test recomputes them from Python integers.  Under every other schedule the outputs must be the
// first schedule's, byte for byte (SCHEDULES same=<n> differ=<n>).
//
//   sim_dz [saturated]     saturated: every data word and every device-resident challenge word p - 1
//   POLY ncoeffs npoints batch | Z 4 | M npoints | COEF b ... | POUT ...
//   DEEP log_N log_b width stride nslots accumulate offset | Z 4 | SLOT column rotation ai vi (caller's order) | AL | CL | COL c ... | PREV | OUT
//   POINT <hex state> -> Z 4 len status | FIELDS <hex state> <words> -> T len status hex | ROWS ...
#include "hip_sim.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#define TOYNI_KERNEL_TEXT_ONLY
#include "toyni_hip.hip"
#include "../emu/contract_case.hpp"

alignas(16) uint32_t air_lds[4];   // named by the kernel section; no kernel that uses it runs here

extern "C" {
extern uint32_t __start_hipsim_lds[] __attribute__((weak)), __stop_hipsim_lds[] __attribute__((weak));
}
void hipsim::poison_shared() {
    for (uint32_t* p = __start_hipsim_lds; p < __stop_hipsim_lds; ++p) *p = 0xDEADBEEFu;
}

static int failures = 0, same = 0, differ = 0;
static bool saturated = false;
static uint64_t sm_state = 0xD2D2D2D2ull;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t draw() {   // {0, 1, p - 1, random}; saturated: p - 1
    if (saturated) return BB_P - 1u;
    const uint64_t k = splitmix();
    return k % 8 == 0 ? 0u : k % 8 == 1 ? 1u : k % 8 == 2 ? BB_P - 1u : (uint32_t)(splitmix() % BB_P);
}
template <class T> struct Aligned {   // `words` elements behind a 16-byte boundary, `off` elements past it
    T* store;
    T* p;
    Aligned(size_t words, size_t off = 0) {
        store = static_cast<T*>(::operator new((words + off + 4) * sizeof(T), std::align_val_t(16)));
        p = store + off;
    }
    ~Aligned() { ::operator delete(store, std::align_val_t(16)); }
    Aligned(const Aligned&) = delete;
};
template <class F>
static void launch(const char* name, dim3 grid, uint32_t block, F&& body) {
    if (!hipsim::launch(name, "", grid, block, body)) ++failures;
}
static void print_words(const char* tag, const uint32_t* w, size_t n) {
    std::printf("%s", tag);
    for (size_t i = 0; i < n; ++i) std::printf(" %u", w[i]);
    std::printf("\n");
}
// runs `once(k)` under every schedule; the outputs (out, bytes) of schedule 0 are printed by the caller afterwards from `first`
template <class F>
static void every_schedule(std::vector<uint8_t>& first, const void* out, size_t bytes, F&& once) {
    for (int k = 0; k < hipsim::NUM_SCHEDULES; ++k) {
        hipsim::st().sched = hipsim::schedule_of(k);
        once();
        if (k == 0) first.assign(static_cast<const uint8_t*>(out), static_cast<const uint8_t*>(out) + bytes);
        else if (!memcmp(first.data(), out, bytes)) ++same;
        else { ++differ; std::printf("DIFFER under %s\n", hipsim::schedule_name(k).c_str()); }
    }
}

static void run_poly(uint64_t ncoeffs, uint32_t npoints, uint32_t batch) {
    TOYNI_CONTRACT_TAG("sim_dz poly ncoeffs=%llu npoints=%u batch=%u", (unsigned long long)ncoeffs, npoints, batch);
    const uint64_t stride = ncoeffs + 3;
    const uint32_t nblocks = (uint32_t)((ncoeffs + POLY_CHUNK - 1) / POLY_CHUNK);
    const size_t partial_words = (size_t)batch * nblocks * npoints * 4;
    Aligned<uint32_t> coeffs(batch * stride), z(4), out((size_t)batch * npoints * 4), buffer(partial_words + sizeof(PolyExtRecord) / 4);
    for (uint64_t i = 0; i < batch * stride; ++i) coeffs.p[i] = i % stride < ncoeffs ? draw() : 0xFFFFFFF0u;
    PolyDzMults m{};
    for (int k = 0; k < 4; ++k) z.p[k] = saturated ? BB_P - 1u : (uint32_t)(splitmix() % BB_P);
    for (uint32_t p = 0; p < npoints; ++p) m.v[p] = saturated ? BB_P - 1u : p == 0 ? 1u : (uint32_t)(splitmix() % BB_P);
    PolyExtDzArgs a{};
    a.coeffs = coeffs.p;
    a.ncoeffs = ncoeffs;
    a.stride = stride;
    a.batch = batch;
    a.npoints = npoints;
    a.nblocks = nblocks;
    a.partial = buffer.p;
    a.out = out.p;
    PolyExtRecord* rec = reinterpret_cast<PolyExtRecord*>(buffer.p + partial_words);
    std::vector<uint8_t> first;
    every_schedule(first, out.p, (size_t)batch * npoints * 16, [&] {
        for (size_t i = 0; i < partial_words + sizeof(PolyExtRecord) / 4; ++i) buffer.p[i] = 0xCDCDCDCDu;
        for (size_t i = 0; i < (size_t)batch * npoints * 4; ++i) out.p[i] = 0xCDCDCDCDu;
        launch("poly_ext_prepare_kernel", dim3(1), TRANSCRIPT_T, [&] { poly_ext_prepare_kernel(z.p, m, npoints, rec); });
        launch("poly_eval_ext_batch_partial_dz_kernel", dim3(nblocks, batch > 2 ? 2 : batch), POLY_THREADS,
               [&] { poly_eval_ext_batch_partial_dz_kernel(a, rec); });   // (two rows of blocks for three columns: the column loop runs twice)
        launch("poly_eval_ext_batch_final_dz_kernel", dim3(batch > 2 ? 2 : batch), POLY_THREADS, [&] { poly_eval_ext_batch_final_dz_kernel(a, rec); });
    });
    std::printf("POLY %llu %u %u\n", (unsigned long long)ncoeffs, npoints, batch);
    print_words("Z", z.p, 4);
    print_words("M", m.v, npoints);
    for (uint32_t b = 0; b < batch; ++b) {
        std::printf("COEF %u", b);
        for (uint64_t i = 0; i < ncoeffs; ++i) std::printf(" %u", coeffs.p[b * stride + i]);
        std::printf("\n");
    }
    print_words("POUT", reinterpret_cast<const uint32_t*>(first.data()), (size_t)batch * npoints * 4);
}

static void run_deep(int log_N, int log_b, uint32_t nslots, bool accumulate, uint32_t off) {
    TOYNI_CONTRACT_TAG("sim_dz deep log_N=%d nslots=%u accumulate=%d off=%u", log_N, nslots, (int)accumulate, off);
    NttPlan plan;
    if (!build_plan(log_N, plan)) { ++failures; return; }
    const uint64_t N = 1ull << log_N, rows = N >> log_b, col_stride = N + 4;
    const uint32_t width = 5, shift = 7u, wN = bb_root_of_unity_host((uint32_t)log_N), nal = nslots + 2, ncl = nslots + 3;
    Aligned<uint32_t> m((size_t)width * col_stride, off), out(4 * N), prev(4 * N), z(4), al(4 * nal), cl(4 * ncl);
    for (size_t k = 0; k < (size_t)width * col_stride; ++k) m.p[k] = k % col_stride < N ? draw() : 0xFFFFFFF0u;
    for (uint64_t i = 0; i < 4 * N; ++i) prev.p[i] = accumulate ? draw() : 0xCDCDCDCDu;
    for (int k = 0; k < 4; ++k) z.p[k] = saturated ? BB_P - 1u : (uint32_t)(splitmix() % BB_P);
    if (!saturated && nslots == 64 && !accumulate) { z.p[0] = bb_mul_host(shift, bb_pow_host(wN, N - 1)); z.p[1] = z.p[2] = z.p[3] = 0; }   // x_i = z at the last point
    for (uint32_t i = 0; i < 4 * nal; ++i) al.p[i] = draw();
    for (uint32_t i = 0; i < 4 * ncl; ++i) cl.p[i] = draw();
    std::vector<toyni_deep_ext_slot> slots(nslots);
    for (uint32_t t = 0; t < nslots; ++t)
        slots[t] = toyni_deep_ext_slot{(uint32_t)(splitmix() % width), t % 3 == 2 ? (uint32_t)(rows - 1) : (uint32_t)(splitmix() % rows),
                                       (uint32_t)(splitmix() % nal), (uint32_t)(splitmix() % ncl)};
    // what toyni_deep_combine_ext_dz_device arranges
    std::vector<DeepExtSlot> sorted(nslots);
    for (uint32_t t = 0; t < nslots; ++t) sorted[t] = DeepExtSlot{slots[t].column, (uint32_t)((uint64_t)slots[t].rotation << log_b), slots[t].alpha_index, slots[t].value_index};
    std::stable_sort(sorted.begin(), sorted.end(), [](const DeepExtSlot& x, const DeepExtSlot& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
    const bool inline_slots = nslots <= DEEP_EXT_INLINE_SLOTS;
    const size_t table_words = (sizeof(DeepExtRecord) + nslots * sizeof(DeepExtTerm)) / 4, words = table_words + (inline_slots ? 0 : nslots * 4);
    Aligned<uint32_t> buffer(words);
    DeepExtRecord* rec = reinterpret_cast<DeepExtRecord*>(buffer.p);
    DeepExtArgs a{};
    a.values = m.p;
    a.out = out.p;
    a.col_stride = col_stride;
    a.dom.dom = sub_domain(plan, plan.fwd.data(), 0);
    a.dom.shiftR = to_mont_host(shift);
    a.log_N = (uint32_t)log_N;
    a.nterms = nslots;
    a.wNR = to_mont_host(wN);
    a.accumulate = accumulate ? 1u : 0u;
    std::vector<uint8_t> first;
    every_schedule(first, out.p, 16 * N, [&] {
        for (size_t i = 0; i < words; ++i) buffer.p[i] = 0xCDCDCDCDu;
        memcpy(out.p, prev.p, 16 * N);
        if (inline_slots) {
            DeepExtInlineSlots in{};
            std::copy(sorted.begin(), sorted.end(), in.s);
            launch("deep_ext_prepare_inline_kernel", dim3(1), TRANSCRIPT_T, [&] { deep_ext_prepare_inline_kernel(in, nslots, z.p, al.p, cl.p, rec); });
        } else {
            DeepExtSlot* d_slots = reinterpret_cast<DeepExtSlot*>(buffer.p + table_words);
            memcpy(d_slots, sorted.data(), nslots * sizeof(DeepExtSlot));
            launch("deep_ext_prepare_kernel", dim3(1), TRANSCRIPT_T, [&] { deep_ext_prepare_kernel(d_slots, nslots, z.p, al.p, cl.p, rec); });
        }
        const uint64_t items = log_N >= 2 ? N / 4 : N;
        launch("deep_combine_ext_dz_kernel", dim3((unsigned)((items + 255) / 256)), 256, [&] { deep_combine_ext_dz_kernel(a, rec); });
    });
    std::printf("DEEP %d %d %u %llu %u %d %u\n", log_N, log_b, width, (unsigned long long)col_stride, nslots, (int)accumulate, off);
    print_words("Z", z.p, 4);
    for (uint32_t t = 0; t < nslots; ++t) std::printf("SLOT %u %u %u %u\n", slots[t].column, slots[t].rotation, slots[t].alpha_index, slots[t].value_index);
    print_words("AL", al.p, 4 * nal);
    print_words("CL", cl.p, 4 * ncl);
    for (uint32_t c = 0; c < width; ++c) {
        std::printf("COL %u", c);
        for (uint64_t i = 0; i < N; ++i) std::printf(" %u", m.p[c * col_stride + i]);
        std::printf("\n");
    }
    print_words("PREV", prev.p, accumulate ? 4 * N : 0);
    print_words("OUT", reinterpret_cast<const uint32_t*>(first.data()), 4 * N);
}

static void run_transcript() {
    alignas(16) static TranscriptState tr;
    for (uint32_t len : {0u, 14u, 55u, 241u}) {
        uint8_t state[241];
        for (uint32_t i = 0; i < len; ++i) state[i] = (uint8_t)(splitmix() & 0xFF);
        const auto reset = [&] {
            memset(&tr, 0, sizeof tr);
            memset(tr.bytes, 0x5A, sizeof tr.bytes);
            memcpy(tr.bytes, state, len);
            tr.len = len;
        };
        const auto hex = [&](const uint8_t* b, uint32_t n) { if (!n) std::printf("-"); for (uint32_t i = 0; i < n; ++i) std::printf("%02x", b[i]); };
        // the point
        Aligned<uint32_t> zp(4);
        std::vector<uint8_t> first;
        uint32_t after[2] = {0, 0};
        every_schedule(first, &tr, sizeof tr, [&] {
            reset();
            launch("transcript_squeeze_ext_point_kernel", dim3(1), TRANSCRIPT_T, [&] { transcript_squeeze_ext_point_kernel(&tr, zp.p); });
            after[0] = tr.len, after[1] = tr.status;
        });
        std::printf("POINT ");
        hex(state, len);
        std::printf(" %u %u %u %u %u %u ", zp.p[0], zp.p[1], zp.p[2], zp.p[3], after[0], after[1]);
        hex(first.data() + 16, after[0]);
        std::printf("\n");
        // absorb_fields: 96 words (four of them in need of the reduction), which 241 bytes of state cannot take
        Aligned<uint32_t> words(96);
        for (uint32_t i = 0; i < 96; ++i) words.p[i] = saturated ? BB_P - 1u : i == 0 ? BB_P : i == 1 ? 0xFFFFFFFFu : i == 2 ? 0u : (uint32_t)splitmix();
        every_schedule(first, &tr, sizeof tr, [&] {
            reset();
            launch("transcript_absorb_fields_kernel", dim3(1), TRANSCRIPT_T, [&] { transcript_absorb_fields_kernel(&tr, words.p, 96u); });
            after[0] = tr.len, after[1] = tr.status;
        });
        std::printf("FIELDS ");
        hex(state, len);
        print_words("", words.p, 96);
        std::printf("T %u %u ", after[0], after[1]);
        hex(first.data() + 16, after[0]);
        std::printf("\n");
    }
    // the rows
    struct Rows { uint64_t n; uint32_t noffsets; uint32_t off[8]; uint32_t count; };
    for (const Rows& r : {Rows{1, 1, {0}, 3}, Rows{1ull << 32, 2, {0, 0xFFFFFFFFu}, 5}, Rows{1 << 14, 2, {0, 4}, 8}, Rows{96, 8, {0, 95, 1, 2, 3, 5, 8, 13}, 700}}) {
        Aligned<uint32_t> idx(r.count), out((size_t)r.count * r.noffsets);
        for (uint32_t i = 0; i < r.count; ++i) idx.p[i] = i == 0 ? 0xFFFFFFFFu : (uint32_t)splitmix();
        QueryRowOffsets off{};
        memcpy(off.v, r.off, sizeof off.v);
        const uint64_t total = (uint64_t)r.count * r.noffsets;
        std::vector<uint8_t> first;
        every_schedule(first, out.p, 4 * total, [&] {
            for (uint64_t i = 0; i < total; ++i) out.p[i] = 0xCDCDCDCDu;
            launch("query_rows_kernel", dim3(2), 256, [&] { query_rows_kernel(idx.p, off, r.noffsets, r.n, total, out.p); });
        });
        std::printf("ROWS %llu %u", (unsigned long long)r.n, r.noffsets);
        print_words("", r.off, r.noffsets);
        print_words("IDX", idx.p, r.count);
        print_words("W", reinterpret_cast<const uint32_t*>(first.data()), total);
    }
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOFBF, 1 << 20);
    saturated = argc > 1 && !strcmp(argv[1], "saturated");
    struct Poly { uint64_t ncoeffs; uint32_t npoints, batch; };
    for (const Poly& p : {Poly{1, 1, 1}, Poly{15, 2, 3}, Poly{16, 3, 1}, Poly{17, 4, 3}, Poly{4095, 1, 3}, Poly{4096, 2, 1}, Poly{4097, 3, 3}, Poly{2 * 4096 + 5, 4, 1}})
        if (!saturated || p.ncoeffs == 17 || p.ncoeffs == 4097) run_poly(p.ncoeffs, p.npoints, p.batch);
    for (int log_N : {1, 2, 10})
        for (uint32_t nslots : {1u, 64u, 65u})
            for (int acc = 0; acc < 2; ++acc)
                for (uint32_t off : {0u, 1u})
                    if (!saturated || (log_N == 10 && nslots >= 64)) run_deep(log_N, log_N == 10 ? 2 : 1, nslots, acc != 0, off);
    run_transcript();
    hipsim::State& s = hipsim::st();
    std::printf("SCHEDULES same=%d differ=%d\nlaunches=%llu launch failures=%d hard failures=%llu\nDONE\n", same, differ, s.launches, failures, s.hard_failures);
    return 0;
}
