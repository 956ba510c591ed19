// Steps the bodies of the Ext accumulator-column kernels (ext_accum_* / ext_tower_inverses / ext_invert_group:
// toyni_amd/csrc/prover_kernels.hpp, include/toyni_hip.h 3i) on the CPU, the way emu_scan.cpp steps those of 3g: workgroup by
// workgroup, wave by wave, the cross-lane steps lane by lane on arrays of 64 values, one per coordinate.  The glue between the bodies
// restates ext_accum_*_kernel of toyni_hip.hip (tests/sim runs the kernels' own text) on a REDUCED tile: groups of 4, workgroups of
// 128 threads = two waves, 512 elements.  Prints
//     SCAN <op> <n> <batch> <num width> <den width> <in place: 0 no, 1 on num, 2 on den> <word offset> <strides: num den out>
//     INIT <4 batch values> / NSHIFT <4> / DSHIFT <4>
//     NUM <b> <k> <n values> / DEN <b> <k> <n values>      (the coordinate columns present, as they were before the call)
//     OUT <b> <k> <n values>
//     TOT <b> <8 words>
//     BINV <count> <word offset> <in place> / IN <k> <values> / INV <k> <values> / ZEROS <z>
// tests/test_emu_scan_ext.py recomputes every word with Python integers.  Every operand owns exactly the words its layout owns, so an
// over-read or an over-write is an AddressSanitizer error; the words between n and a stride hold a value >= p and must keep it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "prover_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;

// `saturated` as the only argument runs, instead of the cases above, the ones whose every product is (p - 1)^2: every data word
// p - 1 and every challenge coordinate SAT_X, the plain value whose Montgomery form is p - 1 (same record format)

constexpr int G = 4, T = 128, NW = T / (int)SCAN_WAVE, TILE = G * T;
constexpr uint32_t SLACK = 0xFFFFFFF0u;

static uint64_t sm_state = 0xE87ACC0Bull;
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

// the workgroup-wide exclusive scan of one zero count per thread, as emu_scan.cpp restates scan_block_exclusive<SCAN_COUNT>
static uint32_t count_total(const uint32_t (&v)[T]) {
    uint32_t total = 0;
    for (int w = 0; w < NW; ++w) {
        uint32_t lanes[SCAN_WAVE];
        for (uint32_t l = 0; l < SCAN_WAVE; ++l) lanes[l] = v[w * SCAN_WAVE + l];
        for (uint32_t delta = 1; delta < SCAN_WAVE; delta <<= 1) {
            uint32_t next[SCAN_WAVE];
            for (uint32_t l = 0; l < SCAN_WAVE; ++l) next[l] = scan_wave_step<SCAN_COUNT>(lanes[l], scan_lane_up(lanes, l, delta), l, delta);
            std::memcpy(lanes, next, sizeof lanes);
        }
        total += lanes[SCAN_WAVE - 1];
    }
    return total;
}
// ext_accum_block_exclusive of toyni_hip.hip
template <int OP>
static Ext4 block_exclusive(const Ext4 (&v)[T], Ext4 (&pre)[T]) {
    Ext4 wave_tot[NW], inc[T];
    for (int w = 0; w < NW; ++w) {                                  // each wave on its own
        uint32_t lanes[4][SCAN_WAVE];
        for (uint32_t l = 0; l < SCAN_WAVE; ++l)
            for (int k = 0; k < 4; ++k) lanes[k][l] = v[w * SCAN_WAVE + l].c[k];
        for (uint32_t delta = 1; delta < SCAN_WAVE; delta <<= 1) {
            uint32_t next[4][SCAN_WAVE];
            for (uint32_t l = 0; l < SCAN_WAVE; ++l) {
                Ext4 mine, below;
                for (int k = 0; k < 4; ++k) { mine.c[k] = lanes[k][l]; below.c[k] = scan_lane_up(lanes[k], l, delta); }
                const Ext4 r = l >= delta ? ext_accum_combine<OP>(below, mine) : mine;
                for (int k = 0; k < 4; ++k) next[k][l] = r.c[k];
            }
            std::memcpy(lanes, next, sizeof lanes);
        }
        for (uint32_t l = 0; l < SCAN_WAVE; ++l)
            for (int k = 0; k < 4; ++k) inc[w * SCAN_WAVE + l].c[k] = lanes[k][l];
        wave_tot[w] = inc[w * SCAN_WAVE + SCAN_WAVE - 1];
    }
    Ext4 total = ext_accum_identity<OP>();                          // (barrier)
    for (int w = 0; w < NW; ++w)
        for (uint32_t l = 0; l < SCAN_WAVE; ++l) {
            const Ext4 p = ext_accum_waves_below<OP, NW>(wave_tot, (uint32_t)w, total);
            pre[w * SCAN_WAVE + l] = l ? ext_accum_combine<OP>(p, inc[w * SCAN_WAVE + l - 1]) : p;
        }
    return total;
}

template <int OP>
static void aggregate_block(const ExtAccumArgs& a, uint32_t col, uint32_t tile) {
    Ext4 v[T], pre[T];
    uint32_t z[T];
    for (int t = 0; t < T; ++t) {
        Ext4 terms[G], ex[G];
        z[t] = ext_accum_group_terms<OP, G>(a, col, (uint64_t)tile * TILE + (uint64_t)t * G, a.n, terms);
        v[t] = ext_accum_thread_serial<OP, G>(terms, ex);
    }
    const Ext4 total = block_exclusive<OP>(v, pre);
    for (int k = 0; k < 4; ++k) ext_accum_tile_aggregates(a, col)[(uint64_t)k * a.ntiles + tile] = total.c[k];
    ext_accum_tile_zeros(a, col)[tile] = count_total(z);
}

static void write_totals(const ExtAccumArgs& a, uint32_t col, const Ext4& tot, uint32_t zeros) {
    if (!a.totals) return;
    for (int k = 0; k < 4; ++k) a.totals[8 * col + k] = tot.c[k];
    a.totals[8 * col + 4] = zeros;
    for (int k = 5; k < 8; ++k) a.totals[8 * col + k] = 0u;
}

template <int OP>
static void prefix_block(const ExtAccumArgs& a, const ExtAccumSeeds& in, uint32_t col) {
    uint32_t* agg = ext_accum_tile_aggregates(a, col);
    Ext4 carry = {{in.v[col][0], in.v[col][1], in.v[col][2], in.v[col][3]}};
    for (uint32_t base = 0; base < a.ntiles; base += TILE) {       // rounds of one tile of aggregates
        static Ext4 v[T], pre[T], ex[T][G];
        for (int t = 0; t < T; ++t) {
            Ext4 terms[G];
            const uint64_t i0 = (uint64_t)base + t * G;
            ext_column_group_load<G>(agg, a.ntiles, i0, a.ntiles, terms);
            for (int j = 0; j < G; ++j)
                if (i0 + (uint64_t)j >= a.ntiles) terms[j] = ext_accum_identity<OP>();
            v[t] = ext_accum_thread_serial<OP, G>(terms, ex[t]);
        }
        const Ext4 total = block_exclusive<OP>(v, pre);
        for (int t = 0; t < T; ++t) {
            Ext4 o[G];
            const Ext4 mine = ext_accum_combine<OP>(carry, pre[t]);
            for (int j = 0; j < G; ++j) o[j] = ext_accum_combine<OP>(mine, ex[t][j]);
            ext_column_group_store<G>(agg, a.ntiles, (uint64_t)base + t * G, a.ntiles, o);
        }
        carry = ext_accum_combine<OP>(carry, total);
    }
    const uint32_t* zc = ext_accum_tile_zeros(a, col);
    uint32_t z[T];
    for (int t = 0; t < T; ++t) {
        z[t] = 0;
        for (uint32_t k = (uint32_t)t; k < a.ntiles; k += T) z[t] += zc[k];
    }
    write_totals(a, col, ext_accum_to_plain<OP>(carry), count_total(z));
}

template <int OP>
static void apply_block(const ExtAccumArgs& a, const ExtAccumSeeds& in, uint32_t col, uint32_t tile) {
    static Ext4 v[T], pre[T], ex[T][G];
    uint32_t z[T];
    for (int t = 0; t < T; ++t) {
        Ext4 terms[G];
        z[t] = ext_accum_group_terms<OP, G>(a, col, (uint64_t)tile * TILE + (uint64_t)t * G, a.n, terms);
        v[t] = ext_accum_thread_serial<OP, G>(terms, ex[t]);
    }
    const Ext4 total = block_exclusive<OP>(v, pre);
    Ext4 seed;
    for (int k = 0; k < 4; ++k) seed.c[k] = a.single ? in.v[col][k] : ext_accum_tile_aggregates(a, col)[(uint64_t)k * a.ntiles + tile];
    for (int t = 0; t < T; ++t) {
        Ext4 o[G];
        ext_accum_group_finish<OP, G>(ext_accum_combine<OP>(seed, pre[t]), ex[t], o);
        ext_column_group_store<G>(a.out + 4ull * col * a.out_stride, a.out_stride, (uint64_t)tile * TILE + (uint64_t)t * G, a.n, o);
    }
    if (a.single) write_totals(a, col, ext_accum_to_plain<OP>(ext_accum_combine<OP>(seed, total)), count_total(z));
}

template <int OP>
static void run_scan(ExtAccumArgs& a, const ExtAccumSeeds& in, uint32_t batch) {
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
static bool zero_at(Zeros zeros, size_t i, size_t n) {
    const size_t in_tile = i % TILE, in_group = i % G;
    if (zeros == Z_EDGES) return in_tile == 0 || in_tile == TILE - 1 || ((i / G) % 3 == 1 && (in_group == 0 || in_group == G - 1)) || i == n - 1;
    if (zeros == Z_GROUP) return (i / G) % 2 == 1;
    return zeros == Z_ALL;
}
static uint32_t neg(uint32_t v) { return v ? BB_P - v : 0u; }
static void print_col(const char* tag, uint32_t b, int k, const uint32_t* v, size_t n) {
    std::printf("%s %u %d", tag, b, k);
    for (size_t i = 0; i < n; ++i) std::printf(" %u", v[i]);
    std::printf("\n");
}
static size_t operand_words(uint32_t width, uint32_t batch, size_t stride, size_t n) { return width ? ((size_t)width * batch - 1) * stride + n : 1; }

static int bad = 0;
// base_shift: the denominator's shift is (s, 0, 0, 0) -- the only shifts under which a width-1 denominator can vanish
static void scan_case(int op, size_t n, uint32_t batch, uint32_t nw, uint32_t dw, int inplace, uint32_t off, Zeros zeros, bool base_shift, bool edges = true,
                      bool sat = false) {
    TOYNI_CONTRACT_TAG("ext_accum op=%d n=%zu batch=%u nw=%u dw=%u inplace=%d sat=%d", op, n, batch, nw, dw, inplace, (int)sat);
    const size_t pad_n = batch > 1 ? 3 : 0, pad_d = batch > 1 ? 5 : 0;
    const size_t ns = n + pad_n, ds = n + pad_d, os = inplace == 1 ? ns : inplace == 2 ? ds : n + (batch > 1 ? 1 : 0);
    Buf num(operand_words(nw, batch, ns, n), off), den(operand_words(dw, batch, ds, n), (off + 1) % 4), out(operand_words(4, batch, os, n), (off + 2) % 4);
    ExtAccumArgs a{};
    for (int k = 0; k < 4; ++k) {
        a.num.shift[k] = nw ? 1u + (uint32_t)(splitmix() % (BB_P - 1)) : 0u;
        a.den.shift[k] = dw && (k == 0 || !base_shift) ? 1u + (uint32_t)(splitmix() % (BB_P - 1)) : 0u;
    }
    for (uint32_t b = 0; b < batch; ++b)
        for (size_t i = 0; i < n; ++i) {
            for (uint32_t k = 0; k < nw; ++k) num.p[(nw * b + k) * ns + i] = edges ? draw(splitmix()) : (uint32_t)(splitmix() % BB_P);
            if (dw == 1) {   // the stored value v; shift + v vanishes only for v = p - s under a base shift
                uint32_t v = edges ? draw(splitmix()) : (uint32_t)(splitmix() % BB_P);
                if (base_shift && v == neg(a.den.shift[0])) v = 1u;
                if (base_shift && zero_at(zeros, i, n)) v = neg(a.den.shift[0]);
                den.p[b * ds + i] = v;
            } else if (dw == 4) {   // the VALUE d = shift + stored is drawn: coordinates from {0, 1, p - 1, random}, not all zero ...
                uint32_t d[4];
                for (int k = 0; k < 4; ++k) d[k] = edges ? draw(splitmix()) : (uint32_t)(splitmix() % BB_P);
                if (i % 7 == 3) d[(i / 7) % 4] = 0u;                                                  // ... one,
                if (i % 7 == 4) d[(i / 7) % 4] = d[(i / 7 + 1) % 4] = 0u;                             // two
                if (i % 7 == 5) d[(i / 7) % 4] = d[(i / 7 + 1) % 4] = d[(i / 7 + 2) % 4] = 0u;        // and three zero coordinates
                if (!(d[0] | d[1] | d[2] | d[3])) d[(i / 7 + 3) % 4] = 1u + (uint32_t)(splitmix() % (BB_P - 1));
                if (zero_at(zeros, i, n)) d[0] = d[1] = d[2] = d[3] = 0u;
                for (int k = 0; k < 4; ++k) den.p[(4 * b + k) * ds + i] = bb_add(d[k], neg(a.den.shift[k]));
            }
        }
    if (sat) {   // gamma = (SAT_X, SAT_X, SAT_X, SAT_X) on both operands, every stored word p - 1
        for (int k = 0; k < 4; ++k) a.num.shift[k] = nw ? SAT_X : 0u, a.den.shift[k] = dw ? SAT_X : 0u;
        for (uint32_t b = 0; b < batch; ++b)
            for (size_t i = 0; i < n; ++i) {
                for (uint32_t k = 0; k < nw; ++k) num.p[(nw * b + k) * ns + i] = BB_P - 1u;
                for (uint32_t k = 0; k < dw; ++k) den.p[(dw * b + k) * ds + i] = BB_P - 1u;
            }
    }
    ExtAccumSeeds in{};
    std::vector<uint32_t> init(4 * batch);
    for (uint32_t b = 0; b < batch; ++b)
        for (int k = 0; k < 4; ++k) {
            init[4 * b + k] = sat ? SAT_X : b == 0 ? (op == (int)SCAN_PRODUCT && k == 0 ? 1u : 0u) : draw(b + 1 + n + k);
            if (op == (int)SCAN_PRODUCT && k == 0 && init[4 * b] == 0u) init[4 * b] = BB_P - 1u;
            in.v[b][k] = op == (int)SCAN_PRODUCT ? to_mont_host(init[4 * b + k]) : init[4 * b + k];
        }
    std::printf("SCAN %d %zu %u %u %u %d %u %zu %zu %zu\nINIT", op, n, batch, nw, dw, inplace, off, ns, ds, os);
    for (uint32_t v : init) std::printf(" %u", v);
    std::printf("\nNSHIFT %u %u %u %u\nDSHIFT %u %u %u %u\n", a.num.shift[0], a.num.shift[1], a.num.shift[2], a.num.shift[3], a.den.shift[0],
                a.den.shift[1], a.den.shift[2], a.den.shift[3]);
    for (uint32_t b = 0; b < batch; ++b) {
        for (uint32_t k = 0; k < nw; ++k) print_col("NUM", b, (int)k, num.p + (nw * b + k) * ns, n);
        for (uint32_t k = 0; k < dw; ++k) print_col("DEN", b, (int)k, den.p + (dw * b + k) * ds, n);
    }
    a.num.values = nw ? num.p : nullptr; a.num.stride = ns; a.num.width = nw;
    a.den.values = dw ? den.p : nullptr; a.den.stride = ds; a.den.width = dw;
    if (dw == 1) {
        const uint32_t z[4] = {neg(a.den.shift[0]), neg(a.den.shift[1]), neg(a.den.shift[2]), neg(a.den.shift[3])};
        a.den_inv = ext_shift_host(z);
    }
    a.out = inplace == 1 ? num.p : inplace == 2 ? den.p : out.p;
    a.out_stride = os;
    a.n = n;
    a.ntiles = (uint32_t)((n + TILE - 1) / TILE);
    a.single = a.ntiles == 1;
    std::vector<uint32_t> tiles(a.single ? 0 : (size_t)EXT_ACCUM_TILE_WORDS * a.ntiles * batch), totals(8 * batch, SLACK);
    a.tiles = tiles.data();
    a.totals = totals.data();
    if (op == (int)SCAN_PRODUCT) run_scan<SCAN_PRODUCT>(a, in, batch);
    else run_scan<SCAN_SUM>(a, in, batch);
    for (uint32_t b = 0; b < batch; ++b) {
        for (int k = 0; k < 4; ++k) {
            print_col("OUT", b, k, a.out + (4 * b + k) * os, n);
            for (size_t i = n; i < os && (4 * b + k + 1) < 4 * batch; ++i) bad += a.out[(4 * b + k) * os + i] != SLACK;   // up to the stride: kept
        }
        std::printf("TOT %u", b);
        for (int k = 0; k < 8; ++k) std::printf(" %u", totals[8 * b + k]);
        std::printf("\n");
    }
}

static void inverse_case(size_t count, uint32_t off, bool inplace, bool sat = false) {
    TOYNI_CONTRACT_TAG("ext_invert_group count=%zu off=%u sat=%d", count, off, (int)sat);
    const size_t is = count + (off % 2 ? 3 : 0), os = inplace ? is : count + 1;
    Buf in(3 * is + count, off), out(3 * os + count, (off + 3) % 4);
    for (size_t i = 0; i < count; ++i) {
        uint32_t d[4];
        for (int k = 0; k < 4; ++k) d[k] = draw(splitmix());
        if (i % 5 == 1) d[i % 4] = d[(i + 1) % 4] = d[(i + 2) % 4] = 0u;
        if (i % 11 == 7 || (count >= (size_t)2 * G && i / G == 1)) d[0] = d[1] = d[2] = d[3] = 0u;   // zeros, and a whole group of them
        for (int k = 0; k < 4; ++k) in.p[k * is + i] = sat ? (i % 3 ? BB_P - 1u : SAT_X) : d[k];
    }
    std::printf("BINV %zu %u %d\n", count, off, (int)inplace);
    for (int k = 0; k < 4; ++k) print_col("IN", 0, k, in.p + k * is, count);
    uint32_t* o = inplace ? in.p : out.p;
    uint32_t zeros = 0;
    for (size_t i0 = 0; i0 < count; i0 += G) zeros += ext_invert_group<G>(in.p, is, o, os, i0, count);   // ext_invert_columns_kernel: one group per thread
    for (int k = 0; k < 4; ++k) {
        print_col("INV", 0, k, o + k * os, count);
        for (size_t i = count; i < os && k < 3; ++i) bad += o[k * os + i] != SLACK;
    }
    std::printf("ZEROS %u\n", zeros);
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "saturated") {
        for (int op : {(int)SCAN_SUM, (int)SCAN_PRODUCT})
            for (size_t n : {(size_t)G + 1, (size_t)TILE + 1}) {
                scan_case(op, n, 1, 4, 4, 0, 0, Z_NONE, false, true, true);
                scan_case(op, n, 3, 1, 1, 0, 0, Z_NONE, false, true, true);
                scan_case(op, n, 1, 4, 0, 0, 0, Z_NONE, false, true, true);
                scan_case(op, n, 1, 0, 4, 0, 0, Z_NONE, false, true, true);
            }
        inverse_case((size_t)TILE + 1, 0, false, true);
        std::printf("BAD %d\nDONE\n", bad);
        return 0;
    }
    const size_t sizes[] = {1, 2, 3, G - 1, G, G + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5};
    const uint32_t widths[8][2] = {{1, 1}, {4, 4}, {1, 4}, {4, 1}, {0, 1}, {0, 4}, {1, 0}, {4, 0}};
    uint32_t k = 0;
    for (int op : {(int)SCAN_SUM, (int)SCAN_PRODUCT})
        for (size_t n : sizes)
            for (int form = 0; form < 8; ++form) {
                ++k;
                const uint32_t nw = widths[form][0], dw = widths[form][1], batch = (k / 8 + form) % 2 ? 3u : 1u;
                const int inplace = k % 3 == 0 && nw == 4 ? 1 : k % 3 == 1 && dw == 4 ? 2 : 0;
                scan_case(op, n, batch, nw, dw, inplace, k % 4, dw ? (Zeros)(k % 3) : Z_NONE, dw == 1 && k % 3 != 0);
            }
    for (int op : {(int)SCAN_SUM, (int)SCAN_PRODUCT}) {
        scan_case(op, TILE + 9, 1, 4, 4, 0, 0, Z_ALL, false);          // every denominator zero
        scan_case(op, TILE + 9, 1, 1, 1, 0, 0, Z_ALL, true);
        scan_case(op, 2 * TILE + 5, 3, 4, 4, 0, 0, Z_EDGES, false);    // every column 16-byte aligned or not by its stride
        scan_case(op, 2 * TILE + 5, 3, 1, 1, 0, 0, Z_EDGES, true);
        for (uint32_t off = 0; off < 4; ++off) scan_case(op, 3 * TILE, 1, 4, 4, (int)off % 3, off, Z_EDGES, false);
    }
    // more tiles than one round of step 2 takes: TILE + 1 of them; random values, no denominators: the listing stays cheap to check
    scan_case((int)SCAN_SUM, (size_t)TILE * TILE + 1, 1, 4, 0, 0, 0, Z_NONE, false, false);
    scan_case((int)SCAN_PRODUCT, (size_t)TILE * TILE + 7, 1, 4, 0, 1, 1, Z_NONE, false, false);
    for (size_t count : {(size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)TILE - 1, (size_t)TILE + 1})
        for (uint32_t off = 0; off < 4; ++off) inverse_case(count, off, (count + off) % 2 == 0);
    std::printf("BAD %d\nDONE\n", bad);
    return 0;
}
