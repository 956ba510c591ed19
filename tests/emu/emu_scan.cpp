// Steps the bodies of the accumulator-column kernels (scan_group_terms, scan_thread_serial, scan_wave_step, scan_waves_below,
// scan_group_finish ...: toyni_amd/csrc/prover_kernels.hpp, include/toyni_hip.h 3g) on the CPU: workgroup by workgroup, wave by
// wave, and inside a wave's cross-lane steps lane by lane on an array of 64 values (the CPU form of scan_lane_up).  The glue between
// the bodies -- which value goes through LDS, where the barriers stand -- restates column_scan_*_kernel of toyni_hip.hip (the schedule
// restated here is checked against the kernels' own in tests/sim) on a REDUCED
// tile (groups of 4, workgroups of 128 threads = two waves: 512 elements), so that every edge is met at a small size.  Prints
//     SCAN <op> <n> <batch> <has_num> <has_den> <in place: 0 no, 1 on num, 2 on den> <word offset> <strides: num den out>
//     INIT <batch values>
//     NUM <b> <n values> / DEN <b> <n values>        (those present, as they were before the call)
//     OUT <b> <n values>
//     TOT <b> <total> <zeros>
//     BINV <count> <word offset> <in place> / IN <values> / INV <values> / ZEROS <k>
// tests/test_emu_scan.py recomputes every word with Python integers.  Every operand owns exactly the words its layout owns, so an
// over-read or an over-write is an AddressSanitizer error; the words between n and a stride hold a value >= p and must keep it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "prover_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;


constexpr int G = 4, T = 128, NW = T / (int)SCAN_WAVE, TILE = G * T;
constexpr uint32_t SLACK = 0xFFFFFFF0u;

static uint64_t sm_state = 0x5CA11AB1Eull;
static uint64_t splitmix() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint32_t draw(uint64_t k) {   // {0, 1, p - 1, random}
    switch (k % 8) {
        case 0: return 0u;
        case 1: return 1u;
        case 2: return BB_P - 1u;
        default: return (uint32_t)(splitmix() % BB_P);
    }
}

// the workgroup-wide exclusive scan of one value per thread: scan_block_exclusive of toyni_hip.hip
template <int OP>
static uint32_t block_exclusive(const uint32_t (&v)[T], uint32_t (&pre)[T]) {
    uint32_t wave_tot[NW], inc[T];
    for (int w = 0; w < NW; ++w) {                                  // each wave on its own
        uint32_t lanes[SCAN_WAVE];
        for (uint32_t l = 0; l < SCAN_WAVE; ++l) lanes[l] = v[w * SCAN_WAVE + l];
        for (uint32_t delta = 1; delta < SCAN_WAVE; delta <<= 1) {
            uint32_t next[SCAN_WAVE];
            for (uint32_t l = 0; l < SCAN_WAVE; ++l) next[l] = scan_wave_step<OP>(lanes[l], scan_lane_up(lanes, l, delta), l, delta);
            std::memcpy(lanes, next, sizeof lanes);
        }
        for (uint32_t l = 0; l < SCAN_WAVE; ++l) inc[w * SCAN_WAVE + l] = lanes[l];
        wave_tot[w] = lanes[SCAN_WAVE - 1];
    }
    uint32_t total = 0;                                             // (barrier)
    for (int w = 0; w < NW; ++w) {
        uint32_t lanes[SCAN_WAVE];
        for (uint32_t l = 0; l < SCAN_WAVE; ++l) lanes[l] = inc[w * SCAN_WAVE + l];
        for (uint32_t l = 0; l < SCAN_WAVE; ++l) {
            const uint32_t up = scan_lane_up(lanes, l, 1);
            const uint32_t p = scan_waves_below<OP, NW>(wave_tot, (uint32_t)w, total);
            pre[w * SCAN_WAVE + l] = l ? scan_combine<OP>(p, up) : p;
        }
    }
    return total;
}

template <int OP>
static void aggregate_block(const ScanArgs& a, uint32_t col, uint32_t tile) {
    uint32_t v[T], z[T], pre[T];
    for (int t = 0; t < T; ++t) {
        uint32_t terms[G], ex[G];
        z[t] = scan_group_terms<OP, G>(a.num ? a.num + col * a.num_stride : nullptr, a.den ? a.den + col * a.den_stride : nullptr,
                                       (uint64_t)tile * TILE + (uint64_t)t * G, a.n, terms);
        v[t] = scan_thread_serial<OP, G>(terms, ex);
    }
    scan_tile_aggregates(a, col)[tile] = block_exclusive<OP>(v, pre);
    scan_tile_zeros(a, col)[tile] = block_exclusive<SCAN_COUNT>(z, pre);
}

template <int OP>
static void prefix_block(const ScanArgs& a, const ScanInit& in, uint32_t col) {
    uint32_t* agg = scan_tile_aggregates(a, col);
    uint32_t carry = in.v[col];
    for (uint32_t base = 0; base < a.ntiles; base += TILE) {       // rounds of one tile of aggregates
        uint32_t v[T], pre[T], ex[T][G];
        for (int t = 0; t < T; ++t) {
            uint32_t terms[G];
            scan_group_load<G>(agg, (uint64_t)base + t * G, a.ntiles, scan_identity<OP>(), terms);
            v[t] = scan_thread_serial<OP, G>(terms, ex[t]);
        }
        const uint32_t total = block_exclusive<OP>(v, pre);
        for (int t = 0; t < T; ++t) {
            uint32_t o[G];
            const uint32_t mine = scan_combine<OP>(carry, pre[t]);
            for (int j = 0; j < G; ++j) o[j] = scan_combine<OP>(mine, ex[t][j]);
            scan_group_store<G>(agg, (uint64_t)base + t * G, a.ntiles, o);
        }
        carry = scan_combine<OP>(carry, total);
    }
    const uint32_t* zc = scan_tile_zeros(a, col);
    uint32_t z[T], pre[T];
    for (int t = 0; t < T; ++t) {
        z[t] = 0;
        for (uint32_t k = (uint32_t)t; k < a.ntiles; k += T) z[t] += zc[k];
    }
    const uint32_t ztotal = block_exclusive<SCAN_COUNT>(z, pre);
    if (a.totals) {
        a.totals[2 * col] = scan_to_plain<OP>(carry);
        a.totals[2 * col + 1] = ztotal;
    }
}

template <int OP>
static void apply_block(const ScanArgs& a, const ScanInit& in, uint32_t col, uint32_t tile) {
    uint32_t v[T], z[T], pre[T], ex[T][G];
    for (int t = 0; t < T; ++t) {                                   // every load of the workgroup ... (in place: before any store)
        uint32_t terms[G];
        z[t] = scan_group_terms<OP, G>(a.num ? a.num + col * a.num_stride : nullptr, a.den ? a.den + col * a.den_stride : nullptr,
                                       (uint64_t)tile * TILE + (uint64_t)t * G, a.n, terms);
        v[t] = scan_thread_serial<OP, G>(terms, ex[t]);
    }
    const uint32_t total = block_exclusive<OP>(v, pre);
    const uint32_t seed = a.single ? in.v[col] : scan_tile_aggregates(a, col)[tile];
    for (int t = 0; t < T; ++t) {
        uint32_t o[G];
        scan_group_finish<OP, G>(scan_combine<OP>(seed, pre[t]), ex[t], o);
        scan_group_store<G>(a.out + col * a.out_stride, (uint64_t)tile * TILE + (uint64_t)t * G, a.n, o);
    }
    if (a.single) {
        const uint32_t ztotal = block_exclusive<SCAN_COUNT>(z, pre);
        if (a.totals) {
            a.totals[2 * col] = scan_to_plain<OP>(scan_combine<OP>(seed, total));
            a.totals[2 * col + 1] = ztotal;
        }
    }
}

template <int OP>
static void run_scan(ScanArgs& a, const ScanInit& in, uint32_t batch) {
    if (a.single) {
        for (uint32_t col = 0; col < batch; ++col) apply_block<OP>(a, in, col, 0);
        return;
    }
    for (uint32_t col = 0; col < batch; ++col)
        for (uint32_t tile = 0; tile < a.ntiles; ++tile) aggregate_block<OP>(a, col, tile);
    for (uint32_t col = 0; col < batch; ++col) prefix_block<OP>(a, in, col);
    for (uint32_t col = batch; col-- > 0;)                          // any order of workgroups: this one runs backwards
        for (uint32_t tile = a.ntiles; tile-- > 0;) apply_block<OP>(a, in, col, tile);
}

struct Buf {   // exactly `words` words, `off` words past a 16-byte boundary
    uint32_t* store;
    uint32_t* p;
    Buf(size_t words, uint32_t off) {
        store = static_cast<uint32_t*>(::operator new((words + off) * sizeof(uint32_t), std::align_val_t(16)));
        p = store + off;
        for (size_t k = 0; k < words; ++k) p[k] = SLACK;
    }
    ~Buf() { ::operator delete(store, std::align_val_t(16)); }
};

enum Zeros { Z_NONE, Z_EDGES, Z_GROUP, Z_ALL };
static void print_col(const char* tag, uint32_t b, const uint32_t* v, size_t n) {
    std::printf("%s %u", tag, b);
    for (size_t i = 0; i < n; ++i) std::printf(" %u", v[i]);
    std::printf("\n");
}

static int bad = 0;
static void scan_case(int op, size_t n, uint32_t batch, bool has_num, bool has_den, int inplace, uint32_t off, Zeros zeros, bool edges = true) {
    TOYNI_CONTRACT_TAG("column_scan op=%d n=%zu batch=%u num=%d den=%d inplace=%d", op, n, batch, (int)has_num, (int)has_den, inplace);
    const size_t pad_n = batch > 1 ? 3 : 0, pad_d = batch > 1 ? 5 : 0;
    const size_t ns = n + pad_n, ds = n + pad_d, os = inplace == 1 ? ns : inplace == 2 ? ds : n + (batch > 1 ? 1 : 0);
    Buf num(has_num ? (batch - 1) * ns + n : 1, off), den(has_den ? (batch - 1) * ds + n : 1, (off + 1) % 4), out((batch - 1) * os + n, (off + 2) % 4);
    for (uint32_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < n; ++i) {
            if (has_num) num.p[b * ns + i] = edges ? draw(splitmix()) : (uint32_t)(splitmix() % BB_P);
            if (has_den) {
                uint32_t d = edges ? draw(splitmix() | 1u) : 1u + (uint32_t)(splitmix() % (BB_P - 1));   // nonzero ...
                const size_t in_tile = i % TILE, in_group = i % G;
                if (zeros == Z_EDGES && (in_tile == 0 || in_tile == TILE - 1 || ((i / G) % 3 == 1 && (in_group == 0 || in_group == G - 1)))) d = 0;
                if (zeros == Z_EDGES && i == n - 1) d = 0;
                if (zeros == Z_GROUP && (i / G) % 2 == 1) d = 0;   // ... every element of every other group
                if (zeros == Z_ALL) d = 0;
                den.p[b * ds + i] = d;
            }
        }
    ScanInit in{};
    std::vector<uint32_t> init(batch);
    for (uint32_t b = 0; b < batch; ++b) {
        init[b] = b == 0 ? (op == (int)SCAN_PRODUCT ? 1u : 0u) : draw(b + 1 + n);
        if (op == (int)SCAN_PRODUCT && init[b] == 0u) init[b] = BB_P - 1u;
        in.v[b] = op == (int)SCAN_PRODUCT ? to_mont_host(init[b]) : init[b];
    }
    std::printf("SCAN %d %zu %u %d %d %d %u %zu %zu %zu\nINIT", op, n, batch, (int)has_num, (int)has_den, inplace, off, ns, ds, os);
    for (uint32_t v : init) std::printf(" %u", v);
    std::printf("\n");
    for (uint32_t b = 0; b < batch; ++b) {
        if (has_num) print_col("NUM", b, num.p + b * ns, n);
        if (has_den) print_col("DEN", b, den.p + b * ds, n);
    }
    ScanArgs a{};
    a.num = has_num ? num.p : nullptr;
    a.den = has_den ? den.p : nullptr;
    a.out = inplace == 1 ? num.p : inplace == 2 ? den.p : out.p;
    a.num_stride = ns; a.den_stride = ds; a.out_stride = os;
    a.n = n;
    a.ntiles = (uint32_t)((n + TILE - 1) / TILE);
    a.single = a.ntiles == 1;
    std::vector<uint32_t> tiles(a.single ? 0 : 2 * (size_t)a.ntiles * batch), totals(2 * batch, SLACK);
    a.tiles = tiles.data();
    a.totals = totals.data();
    if (op == (int)SCAN_PRODUCT) run_scan<SCAN_PRODUCT>(a, in, batch);
    else run_scan<SCAN_SUM>(a, in, batch);
    for (uint32_t b = 0; b < batch; ++b) {
        print_col("OUT", b, a.out + b * os, n);
        std::printf("TOT %u %u %u\n", b, totals[2 * b], totals[2 * b + 1]);
        for (size_t i = n; i < os && b + 1 < batch; ++i) bad += a.out[b * os + i] != SLACK;   // the words up to the stride keep their value
    }
}

static void inverse_case(size_t count, uint32_t off, bool inplace) {
    TOYNI_CONTRACT_TAG("batch_inverse count=%zu off=%u inplace=%d", count, off, (int)inplace);
    Buf in(count, off), out(count, (off + 3) % 4);
    for (size_t i = 0; i < count; ++i) in.p[i] = draw(splitmix());
    if (count >= (size_t)2 * G) for (int j = 0; j < G; ++j) in.p[G + j] = 0;   // a whole group of zeros
    std::printf("BINV %zu %u %d\nIN", count, off, (int)inplace);
    for (size_t i = 0; i < count; ++i) std::printf(" %u", in.p[i]);
    uint32_t* o = inplace ? in.p : out.p;
    uint32_t zeros = 0;
    for (size_t i0 = 0; i0 < count; i0 += G) {                      // batch_inverse_kernel: one group per thread
        uint32_t t[G];
        zeros += scan_group_terms<SCAN_SUM, G>(nullptr, in.p, i0, count, t);
        scan_group_store<G>(o, i0, count, t);
    }
    std::printf("\nINV");
    for (size_t i = 0; i < count; ++i) std::printf(" %u", o[i]);
    std::printf("\nZEROS %u\n", zeros);
}

int main() {
    const size_t sizes[] = {1, 2, 3, G - 1, G, G + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5};
    uint32_t k = 0;
    for (int op : {(int)SCAN_SUM, (int)SCAN_PRODUCT})
        for (size_t n : sizes)
            for (int form = 0; form < 3; ++form)                    // both operands, no numerators, no denominators
                for (uint32_t batch : {1u, 3u}) {
                    ++k;
                    const bool has_num = form != 1, has_den = form != 2;
                    const int inplace = k % 3 == 0 ? (has_num ? 1 : 2) : k % 3 == 1 && has_den ? 2 : 0;
                    scan_case(op, n, batch, has_num, has_den, inplace, k % 4, has_den ? (Zeros)(k % 3) : Z_NONE);
                }
    for (int op : {(int)SCAN_SUM, (int)SCAN_PRODUCT}) {
        scan_case(op, TILE + 9, 1, true, true, 0, 0, Z_ALL);        // every denominator zero
        scan_case(op, 2 * TILE + 5, 3, true, true, 0, 0, Z_EDGES);  // every column 16-byte aligned or not by its stride
        for (uint32_t off = 0; off < 4; ++off) scan_case(op, 3 * TILE, 1, true, true, (int)off % 3, off, Z_EDGES);
    }
    // more tiles than one round of step 2 takes: TILE + 1 of them; random values without zeros keep the listing short of edge cases
    scan_case((int)SCAN_SUM, (size_t)TILE * TILE + 1, 1, true, true, 0, 0, Z_NONE, false);
    scan_case((int)SCAN_PRODUCT, (size_t)TILE * TILE + 7, 1, true, false, 1, 1, Z_NONE, false);
    for (size_t count : {(size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)TILE - 1, (size_t)TILE + 1})
        for (uint32_t off = 0; off < 4; ++off) inverse_case(count, off, (count + off) % 2 == 0);
    std::printf("BAD %d\nDONE\n", bad);
    return 0;
}
