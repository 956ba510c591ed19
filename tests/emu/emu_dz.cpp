// Steps the z-dependent preparation of include/toyni_hip.h 3o (toyni_amd/csrc/dz_kernels.hpp: the text the one-wave kernels run) on the
// CPU.  TEST INFRASTRUCTURE (tests/test_emu_dz.py builds it under AddressSanitizer + UBSan; tests/test_field_contracts_dz.py rebuilds
// it with tests/emu/field_contracts.hpp in front).  Every input and output lives in a heap block of exactly its size.
//
// Part 1 (no stdin needed, argument `prepare` or `saturated`): for a list of z the records of both preparations are compared with
// memcmp against what the HOST code of the host-argument entry points builds for the same values -- ext_pow_host,
// poly_ext_powers_host, ext_shift_host and the table loop of toyni_deep_combine_ext_device, restated in host_table below -- and the
// raw inputs and outputs are printed for the test to judge against Python integers:
//   PREP z0..z3 mult  |  PW <144 words: thread table, chunk table>   one pair per (z, multiplier)
//   SHIFT z0..z3      |  SH <16 words>
//   DEEP nslots nlanes |  SLOT column rot ai vi (sorted, per slot)  |  AL <words>  |  CL <words>  |  REC <4 claim words>  |  TAB <8 words per slot>
// Part 2 (commands on stdin, argument `transcript`): the transcript helpers and the query rows
//   init <hex|->  |  status <v>  |  fields <lanes> <w0> <w1> ...  |  point -> Z z0 z1 z2 z3  |  state -> T len status hex
//   rows <n> <noffsets> <off...> : <idx...>  -> W r0 r1 ...
// The accept predicate of the point rule is replaced below by one that a global switch drives, so that the rejection branch and the
// bound of 8 tries run: `reject <k>` makes the next k candidates fail (k >= 8: the bound).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

static unsigned g_reject = 0;
static bool dz_test_accept(const unsigned* z) {
    if (g_reject) { --g_reject; return false; }
    return (z[1] | z[2] | z[3]) != 0u;
}
#define TOYNI_DZ_POINT_ACCEPT(z) dz_test_accept(z)
#include "dz_kernels.hpp"
#include "contract_case.hpp"

using namespace toyni;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state += 0x9E3779B97F4A7C15ull;
    uint64_t x = rng_state;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((x ^ (x >> 31)) % BB_P);
}

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return v;
}
template <class T> static void print_words(const char* tag, const T* p, size_t bytes) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
    printf("%s", tag);
    for (size_t i = 0; i < bytes / 4; ++i) printf(" %u", w[i]);
    printf("\n");
}

// what toyni_poly_eval_ext_batch_device builds for one point
static void host_powers(const uint32_t point[4], PolyExtPowers& thread, PolyExtPowers& chunk) {
    uint32_t z16[4], zchunk[4], zstride[4];
    ext_pow_host(point, POLY_PER_THREAD, z16);
    ext_pow_host(point, POLY_CHUNK, zchunk);
    ext_pow_host(zchunk, POLY_THREADS, zstride);
    thread = poly_ext_powers_host(point, z16);
    chunk = poly_ext_powers_host(zstride, zchunk);
}
// what toyni_deep_combine_ext_device builds from host terms: the sorted table and the claim
struct HostTerm { uint32_t column, rot, alpha[4], value[4]; };
static void host_table(const std::vector<HostTerm>& terms, std::vector<DeepExtTerm>& table, uint32_t claim[4]) {
    table.assign(terms.size(), DeepExtTerm{});
    for (int k = 0; k < 4; ++k) claim[k] = 0;
    for (size_t t = 0; t < terms.size(); ++t) {
        DeepExtTerm& e = table[t];
        e.column = terms[t].column;
        e.rot = terms[t].rot;
        uint32_t av[4];
        ext_mul_host(terms[t].alpha, terms[t].value, av);
        for (int k = 0; k < 4; ++k) {
            e.alphaR[k] = to_mont_host(terms[t].alpha[k]);
            claim[k] = (uint32_t)(((uint64_t)claim[k] + av[k]) % BB_P);
        }
    }
    std::stable_sort(table.begin(), table.end(), [](const DeepExtTerm& x, const DeepExtTerm& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
}

static int prepare(bool saturated) {
    int bad = 0;
    std::vector<std::vector<uint32_t>> zs;
    if (saturated) {
        zs.push_back({BB_P - 1, BB_P - 1, BB_P - 1, BB_P - 1});
    } else {
        for (int i = 0; i < 6; ++i) zs.push_back({rnd(), rnd(), rnd(), rnd()});
        zs.push_back({rnd(), 0u, rnd(), rnd()});                        // a zero coordinate
        zs.push_back({rnd(), 0u, 0u, 0u});                              // in the base field
        zs.push_back({0u, 0u, 0u, 0u});
        zs.push_back({BB_P - 1, BB_P - 1, BB_P - 1, BB_P - 1});
        zs.push_back({1u, 0u, 0u, 0u});
    }
    const uint32_t g = bb_root_of_unity_host(10);
    for (const auto& zv : zs) {
        std::unique_ptr<uint32_t[]> z(new uint32_t[4]);
        memcpy(z.get(), zv.data(), 16);
        // ---- the two tables per point, multipliers 1 and g (saturated: p - 1) ----
        for (uint32_t mult : {1u, saturated ? BB_P - 1 : g}) {
            TOYNI_CONTRACT_TAG("emu_dz powers z0=%u mult=%u", z[0], mult);
            uint32_t point[4];
            for (int k = 0; k < 4; ++k) point[k] = bb_mul_host(z[k], mult);
            std::unique_ptr<PolyExtRecord> rec(new PolyExtRecord);
            memset(rec.get(), 0xA5, sizeof(PolyExtRecord));
            poly_ext_record_point(z.get(), mult, rec->thread[1], rec->chunk[2]);
            PolyExtPowers th, ch;
            host_powers(point, th, ch);
            if (memcmp(&th, &rec->thread[1], sizeof th) || memcmp(&ch, &rec->chunk[2], sizeof ch)) { ++bad; printf("MISMATCH powers\n"); }
            printf("PREP %u %u %u %u %u\n", z[0], z[1], z[2], z[3], mult);
            printf("PW");
            for (const PolyExtPowers* pw : {&rec->thread[1], &rec->chunk[2]})
                for (size_t i = 0; i < sizeof(PolyExtPowers) / 4; ++i) printf(" %u", reinterpret_cast<const uint32_t*>(pw)[i]);
            printf("\n");
        }
        // ---- ExtShift ----
        {
            TOYNI_CONTRACT_TAG("emu_dz shift z0=%u", z[0]);
            const ExtShift dev = ext_shift_dev(dz_load_ext(z.get()));
            const ExtShift host = ext_shift_host(z.get());
            if (memcmp(&dev, &host, sizeof dev)) { ++bad; printf("MISMATCH shift\n"); }
            printf("SHIFT %u %u %u %u\n", z[0], z[1], z[2], z[3]);
            print_words("SH", &dev, sizeof dev);
        }
        // ---- the record and the table of the DEEP combination: 1, 5, 64, 65 and 130 slots, stepped as a wave of 1 and of 64 lanes ----
        for (uint32_t nslots : {1u, 5u, 64u, 65u, 130u}) {
            const uint32_t nal = saturated ? 3 : nslots + 2, ncl = saturated ? 2 : nslots + 3;
            std::unique_ptr<uint32_t[]> al(new uint32_t[4 * nal]), cl(new uint32_t[4 * ncl]);
            for (uint32_t i = 0; i < 4 * nal; ++i) al[i] = saturated ? BB_P - 1 : (i % 7 == 0 ? 0u : i % 11 == 0 ? BB_P - 1 : rnd());
            for (uint32_t i = 0; i < 4 * ncl; ++i) cl[i] = saturated ? BB_P - 1 : (i % 5 == 0 ? BB_P - 1 : i % 13 == 0 ? 0u : rnd());
            std::vector<HostTerm> terms(nslots);
            std::vector<DeepExtSlot> slots(nslots);
            for (uint32_t t = 0; t < nslots; ++t) {
                const uint32_t ai = rnd() % nal, vi = rnd() % ncl;
                slots[t] = DeepExtSlot{rnd() % 9u, (rnd() % 4u) * 8u, ai, vi};
                terms[t].column = slots[t].column;
                terms[t].rot = slots[t].rot;
                memcpy(terms[t].alpha, al.get() + 4 * ai, 16);
                memcpy(terms[t].value, cl.get() + 4 * vi, 16);
            }
            // the entry point sorts the slots as the host-argument call sorts its table
            std::stable_sort(slots.begin(), slots.end(), [](const DeepExtSlot& x, const DeepExtSlot& y) { return x.column != y.column ? x.column < y.column : x.rot < y.rot; });
            std::vector<DeepExtTerm> want;
            uint32_t claim[4];
            host_table(terms, want, claim);
            const ExtShift shift = ext_shift_host(z.get());
            for (uint32_t nlanes : {1u, 64u}) {
                TOYNI_CONTRACT_TAG("emu_dz deep z0=%u nslots=%u nlanes=%u", z[0], nslots, nlanes);
                const size_t bytes = sizeof(DeepExtRecord) + nslots * sizeof(DeepExtTerm);
                DeepExtRecord* rec = static_cast<DeepExtRecord*>(aligned_alloc(16, bytes));
                memset(rec, 0xA5, bytes);
                std::unique_ptr<DeepExtSlot[]> sl(new DeepExtSlot[nslots]);
                memcpy(sl.get(), slots.data(), nslots * sizeof(DeepExtSlot));
                std::unique_ptr<uint32_t[]> part(new uint32_t[4 * nlanes]);
                // the lanes of the wave in lock step is what the hardware does; stepping them from the last to lane 0 keeps the one
                // order the text depends on (lane 0 reads the shares after every lane has stored its own)
                for (uint32_t lane = nlanes; lane-- > 0;) deep_ext_prepare(sl.get(), nslots, z.get(), al.get(), cl.get(), rec, part.get(), lane, nlanes);
                if (memcmp(rec->claim, claim, 16) || memcmp(&rec->shift, &shift, sizeof shift) ||
                    memcmp(deep_ext_record_table(rec), want.data(), nslots * sizeof(DeepExtTerm))) { ++bad; printf("MISMATCH deep\n"); }
                if (nlanes == 64u) {
                    printf("DEEP %u %u %u %u %u %u\n", nslots, nal, z[0], z[1], z[2], z[3]);
                    for (uint32_t t = 0; t < nslots; ++t) printf("SLOT %u %u %u %u\n", sl[t].column, sl[t].rot, sl[t].alpha_index, sl[t].value_index);
                    print_words("AL", al.get(), 16 * nal);
                    print_words("CL", cl.get(), 16 * ncl);
                    print_words("REC", rec->claim, 16);
                    print_words("TAB", deep_ext_record_table(rec), nslots * sizeof(DeepExtTerm));
                }
                free(rec);
            }
        }
    }
    printf("BAD %d\nDONE\n", bad);
    return bad ? 1 : 0;
}

static int transcript() {
    TranscriptState* tr = static_cast<TranscriptState*>(aligned_alloc(16, sizeof(TranscriptState)));
    memset(tr, 0, sizeof *tr);
    std::string line;
    unsigned long lineno = 0;
    while (std::getline(std::cin, line)) {
        ++lineno;
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        TOYNI_CONTRACT_TAG("emu_dz line %lu: %s", lineno, cmd.c_str());
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
        } else if (cmd == "reject") {
            in >> g_reject;
        } else if (cmd == "fields") {
            uint32_t lanes = 1;
            unsigned long long v;
            in >> lanes;
            std::vector<uint32_t> w;
            while (in >> v) w.push_back((uint32_t)v);
            std::unique_ptr<uint32_t[]> src(new uint32_t[w.size() ? w.size() : 1]);
            if (!w.empty()) memcpy(src.get(), w.data(), 4 * w.size());
            // every lane reads length and status before lane 0 stores either: lane 0 last
            for (uint32_t lane = lanes; lane-- > 0;) transcript_absorb_fields_wave(*tr, src.get(), (uint32_t)w.size(), lane, lanes);
        } else if (cmd == "point") {
            std::unique_ptr<uint32_t[]> z(new uint32_t[4]);
            for (int k = 0; k < 4; ++k) z[k] = 0xDEADBEEFu;
            transcript_squeeze_ext_point(*tr, z.get());
            printf("Z %u %u %u %u\n", z[0], z[1], z[2], z[3]);
        } else if (cmd == "state") {
            printf("T %u %u ", tr->len, tr->status);
            for (uint32_t k = 0; k < TRANSCRIPT_CAPACITY; ++k) printf("%02x", tr->bytes[k]);
            printf("\n");
        } else if (cmd == "rows") {
            unsigned long long n = 0, v;
            uint32_t noffsets = 0;
            in >> n >> noffsets;
            QueryRowOffsets off{};
            for (uint32_t r = 0; r < noffsets; ++r) { in >> v; off.v[r] = (uint32_t)v; }
            std::string colon;
            in >> colon;
            std::vector<uint32_t> idx;
            while (in >> v) idx.push_back((uint32_t)v);
            std::unique_ptr<uint32_t[]> src(new uint32_t[idx.size()]);
            memcpy(src.get(), idx.data(), 4 * idx.size());
            printf("W");
            for (uint64_t t = 0; t < (uint64_t)idx.size() * noffsets; ++t) printf(" %u", query_row(src.get(), off, noffsets, n, t));
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

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "prepare") return prepare(false);
    if (mode == "saturated") return prepare(true);
    if (mode == "transcript") return transcript();
    fprintf(stderr, "usage: emu_dz prepare | saturated | transcript\n");
    return 2;
}
