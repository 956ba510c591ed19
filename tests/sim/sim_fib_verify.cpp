// Runs the kernels of include/toyni_hip.h 3t themselves -- the five kernels of toyni_amd/csrc/verify/toyni_hip_verify.hip -- on the CPU
// through hip_sim.hpp (unchanged), every GPU thread a fiber, under the eight wave / lane schedules of that header: the proofs of one
// launch lie a stride apart with guard bands between the images, between the proofs' parts of the work buffer and around the verdicts.
//
// TEST INFRASTRUCTURE (tests/test_sim_fib_verify.py; tests/test_field_contracts_fib_verify.py rebuilds it with
// tests/emu/field_contracts.hpp in front).  The images come from the test: a file of  u32 trace_len | u32 batch | batch images of
// toyni_fib_proof_image_bytes(trace_len) bytes.  The arguments of the kernels are built here from trace_len alone, by the arithmetic
// of toyni_fib_proof_layout_of restated; the judge is the test (tests/harness/fib_verifier.py on the same proofs).
//   sim_fib_verify FILE                  the chain under all eight schedules; prints VERDICTS / FLAGS (of the first schedule; every later
//                                        schedule must write the same words), RAN / SITE lines; exit 1 on a failure
//   sim_fib_verify FILE --drop K:i       with the i-th synchronisation site of kernel K switched off: DROP ... FAILS / SURVIVES, where
//                                        FAILS = a hard failure or words that differ from the undisturbed run's
#include "hip_sim.hpp"

#include <cstdio>
#include <cstring>
#include <new>
#include <set>
#include <string>
#include <vector>

#define TOYNI_KERNEL_TEXT_ONLY
#include "verify/toyni_hip_verify.hip"
#include "../emu/contract_case.hpp"

extern "C" {
extern uint32_t __start_hipsim_lds[] __attribute__((weak)), __stop_hipsim_lds[] __attribute__((weak));
}
void hipsim::poison_shared() {
    for (uint32_t* p = __start_hipsim_lds; p < __stop_hipsim_lds; ++p) *p = 0xDEADBEEFu;
}

static int failures = 0;
static std::set<std::string> instantiations;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class F>
static bool sim_launch(const char* name, dim3 grid, uint32_t block, F&& body) {
    instantiations.insert(name);
    TOYNI_CONTRACT_TAG("%s", name);
    const bool ok = hipsim::launch(name, "", grid, block, body);
    if (!ok) ++failures;
    return ok;
}

constexpr uint32_t FILL = 0xCDCDCDCDu;
constexpr size_t GUARD = 8;   // words

static unsigned ceil_log2(size_t v) { unsigned l = 0; while (((size_t)1 << l) < v) ++l; return l; }

struct Shape {
    FibVerifyArgs a{};
    size_t image_bytes = 0;
    size_t leaves[VERIFY_MAX_GROUPS] = {}, records[VERIFY_MAX_GROUPS] = {};
};
// toyni_fib_proof_layout_of, restated
static Shape shape_of(size_t n) {
    Shape s;
    FibVerifyArgs& a = s.a;
    const size_t N = n << FIBV_LOG_BLOWUP, Q = FIBV_QUERIES;
    size_t C = 1;
    while (C < n + FIBV_MASK_DEGREE) C <<= 1;
    a.log_n = ceil_log2(n);
    a.log_N = a.log_n + FIBV_LOG_BLOWUP;
    a.folds = ceil_log2(C);
    a.final_size = (uint32_t)(N / C);
    const size_t ood = 32 * (a.folds + 3), idx = ood + 16, fin = idx + 4 * Q;
    size_t at = (fin + 4 * a.final_size + 7) & ~(size_t)7;
    a.ood_word = (uint32_t)(ood / 4);
    a.index_word = (uint32_t)(idx / 4);
    a.final_word = (uint32_t)(fin / 4);
    a.ngroups = a.folds + 2;
    for (uint32_t g = 0; g < a.ngroups; ++g) {
        s.leaves[g] = g < 3 ? N : N >> (g - 2);
        s.records[g] = g == 0 ? 3 * Q : g == 1 ? Q : 2 * Q;
        a.group_depth[g] = ceil_log2(s.leaves[g]);
        a.group_byte[g] = at;
        a.group_first[g + 1] = a.group_first[g] + (uint32_t)s.records[g];
        at += s.records[g] * verify_record_bytes(a.group_depth[g]);
    }
    for (uint32_t g = a.ngroups + 1; g <= VERIFY_MAX_GROUPS; ++g) a.group_first[g] = a.group_first[a.ngroups];
    a.nrecords = a.group_first[a.ngroups];
    s.image_bytes = (at + 15) & ~(size_t)15;
    const uint32_t g_inv = bb_inv_host(bb_root_of_unity_host(a.log_n));
    a.b1R = to_mont_host(g_inv);
    a.b2R = to_mont_host(bb_mul_host(g_inv, g_inv));
    a.shift_invR = to_mont_host(bb_inv_host(FIBV_SHIFT));
    a.wNR = to_mont_host(bb_root_of_unity_host(a.log_N));
    return s;
}

struct Result { std::vector<uint32_t> verdicts, flags; };

// the chain of toyni_fib_verify_batch_device, launch for launch
static Result run_chain(const Shape& sh, const std::vector<uint8_t>& file_images, size_t batch) {
    FibVerifyArgs a = sh.a;
    const size_t image_words = sh.image_bytes / 4;
    a.image_stride = sh.image_bytes + 16 * 3;                                   // a gap of 48 bytes behind every image
    const size_t work_extent = FIBV_W_POS + 2 * (size_t)a.nrecords;
    a.work_stride = (work_extent + 3 + GUARD) & ~(size_t)3;
    const size_t img_total = batch * a.image_stride / 4, work_total = batch * a.work_stride, out_total = batch + 2 * GUARD;
    uint32_t* img = static_cast<uint32_t*>(::operator new(img_total * 4, std::align_val_t(16)));
    uint32_t* work = static_cast<uint32_t*>(::operator new(work_total * 4, std::align_val_t(16)));
    uint32_t* out = static_cast<uint32_t*>(::operator new(out_total * 4, std::align_val_t(16)));
    for (size_t i = 0; i < img_total; ++i) img[i] = FILL;
    for (size_t i = 0; i < work_total; ++i) work[i] = FILL;
    for (size_t i = 0; i < out_total; ++i) out[i] = FILL;
    for (size_t b = 0; b < batch; ++b) std::memcpy(reinterpret_cast<uint8_t*>(img) + b * a.image_stride, file_images.data() + b * sh.image_bytes, sh.image_bytes);
    std::vector<uint32_t> img_before(img, img + img_total);
    const uint8_t* images = reinterpret_cast<const uint8_t*>(img);
    uint32_t* verdicts = out + GUARD;

    sim_launch("fib_verify_replay_kernel", dim3((unsigned)batch), VERIFY_WAVE, [&] { fib_verify_replay_kernel(a, images, work); });
    sim_launch("fib_verify_global_kernel", dim3((unsigned)batch), VERIFY_WAVE, [&] { fib_verify_global_kernel(a, images, work); });
    MerkleVerifyGroups gs{};
    gs.ngroups = a.ngroups;
    gs.batch = (uint32_t)batch;
    for (uint32_t g = 0; g < a.ngroups; ++g) {
        gs.records[g] = images + a.group_byte[g];
        gs.record_stride[g] = a.image_stride;
        gs.indices[g] = work + FIBV_W_POS + a.group_first[g];
        gs.index_stride[g] = a.work_stride;
        gs.root[g] = images + 32u * g;
        gs.root_stride[g] = a.image_stride;
        gs.flags[g] = work + FIBV_W_POS + a.nrecords + a.group_first[g];
        gs.flag_stride[g] = a.work_stride;
        gs.leaves[g] = sh.leaves[g];
        gs.depth[g] = a.group_depth[g];
        gs.salted[g] = 1u;
        gs.first[g + 1] = gs.first[g] + sh.records[g];
    }
    for (uint32_t g = a.ngroups + 1; g <= VERIFY_MAX_GROUPS; ++g) gs.first[g] = gs.first[a.ngroups];
    const uint64_t items = gs.first[a.ngroups] * batch;
    sim_launch("merkle_verify_records_batch_kernel", dim3((unsigned)((items + 255) / 256 > 5 ? 5 : (items + 255) / 256)), 256,
               [&] { merkle_verify_records_batch_kernel(gs); });   // five blocks: the grid-stride loop runs
    sim_launch("fib_verify_query_kernel", dim3((unsigned)batch), VERIFY_WAVE, [&] { fib_verify_query_kernel(a, images, work); });
    sim_launch("fib_verify_verdict_kernel", dim3((unsigned)batch), VERIFY_WAVE, [&] { fib_verify_verdict_kernel(work, a.work_stride, verdicts); });

    CHECK(!std::memcmp(img, img_before.data(), img_total * 4), "the images were written");
    for (size_t b = 0; b < batch; ++b)
        for (size_t i = b * a.work_stride + work_extent; i < (b + 1) * a.work_stride; ++i)
            if (work[i] != FILL) { CHECK(false, "work buffer: the gap behind proof %zu was written at word %zu", b, i); break; }
    for (size_t i = 0; i < GUARD; ++i) CHECK(out[i] == FILL && out[GUARD + batch + i] == FILL, "the guard bands around the verdicts were written");
    (void)image_words;
    Result r;
    r.verdicts.assign(verdicts, verdicts + batch);
    for (size_t b = 0; b < batch; ++b) {
        const uint32_t* f = work + b * a.work_stride + FIBV_W_POS + a.nrecords;
        r.flags.insert(r.flags.end(), f, f + a.nrecords);
    }
    ::operator delete(img, std::align_val_t(16));
    ::operator delete(work, std::align_val_t(16));
    ::operator delete(out, std::align_val_t(16));
    return r;
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    hipsim::State& s = hipsim::st();
    bool drop = false;
    std::string path, only;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--drop") && i + 1 < argc) {
            const char* colon = std::strrchr(argv[++i], ':');
            if (!colon) { std::printf("usage: --drop kernel:ordinal\n"); return 2; }
            only = std::string((const char*)argv[i], (const char*)colon);
            s.drop_kernel = only;
            s.drop_site = std::atoi(colon + 1);
            drop = true;
        } else if (path.empty()) path = argv[i];
        else { std::printf("usage: sim_fib_verify FILE [--drop kernel:ordinal]\n"); return 2; }
    }
    FILE* f = path.empty() ? nullptr : std::fopen(path.c_str(), "rb");
    uint32_t head[2] = {0, 0};
    if (!f || std::fread(head, 4, 2, f) != 2) { std::printf("cannot read %s\n", path.c_str()); return 2; }
    const size_t n = head[0], batch = head[1];
    if (n < 8 || n > (1u << 12) || (n & (n - 1)) || batch < 1 || batch > 256) { std::printf("trace_len %zu / batch %zu: not for this driver\n", n, batch); return 2; }
    const Shape sh = shape_of(n);
    std::vector<uint8_t> images(batch * sh.image_bytes);
    if (std::fread(images.data(), 1, images.size(), f) != images.size() || std::fgetc(f) != EOF) { std::printf("%s: not %zu images of %zu bytes\n", path.c_str(), batch, sh.image_bytes); return 2; }
    std::fclose(f);
    std::printf("SHAPE trace_len=%zu folds=%u final_size=%u nrecords=%u image_bytes=%zu\n", n, sh.a.folds, sh.a.final_size, sh.a.nrecords, sh.image_bytes);

    Result first;
    if (drop) {   // the undisturbed words, under the first schedule
        hipsim::State& st = hipsim::st();
        const std::string k = st.drop_kernel;
        st.drop_kernel.clear();
        st.sched = hipsim::schedule_of(0);
        first = run_chain(sh, images, batch);
        st.drop_kernel = k;
        if (failures) { std::printf("the undisturbed run failed\n"); return 2; }
    }
    for (int k = 0; k < hipsim::NUM_SCHEDULES; ++k) {
        s.sched = hipsim::schedule_of(k);
        const int before = failures;
        const Result r = run_chain(sh, images, batch);
        if (k == 0 && !drop) first = r;
        CHECK(r.verdicts == first.verdicts, "the verdicts differ from the first schedule's");
        CHECK(r.flags == first.flags, "the record words differ from the first schedule's");
        std::printf("SCHEDULE %s failures=%d\n", hipsim::schedule_name(k).c_str(), failures - before);
        if (drop && failures) {
            const hipsim::KernelSites& ks = s.kernels[only];
            if ((size_t)s.drop_site < ks.sites.size()) {
                s.cur_kernel = &s.kernels[only];
                std::printf("DROP %s:%d %s FAILS under %s (%s)\n", only.c_str(), s.drop_site, hipsim::site_text(s.drop_site).c_str(), hipsim::schedule_name(k).c_str(),
                            s.hard_failures ? "hard failure" : "mismatch");
            }
            return 0;
        }
    }
    std::printf("VERDICTS");
    for (uint32_t v : first.verdicts) std::printf(" %u", v);
    std::printf("\n");
    for (size_t b = 0; b < batch; ++b) {
        std::printf("FLAGS %zu ", b);
        for (uint32_t t = 0; t < sh.a.nrecords; ++t) std::printf("%c", first.flags[b * sh.a.nrecords + t] == 1u ? '1' : first.flags[b * sh.a.nrecords + t] == 0u ? '0' : '?');
        std::printf("\n");
    }
    for (const std::string& inst : instantiations) std::printf("RAN %s\n", inst.c_str());
    for (auto& kv : s.kernels) {
        s.cur_kernel = &kv.second;
        for (size_t i = 0; i < kv.second.sites.size(); ++i)
            std::printf("SITE %s:%zu %s arrivals=%llu\n", kv.first.c_str(), i, hipsim::site_text((int)i).c_str(), kv.second.sites[i].arrivals);
    }
    std::printf("launches=%llu fiber switches=%llu hard failures=%llu\n", s.launches, s.switches, s.hard_failures);
    if (drop) {
        if ((size_t)s.drop_site >= s.kernels[only].sites.size()) { std::printf("DROP %s:%d NO SUCH SITE\n", only.c_str(), s.drop_site); return 2; }
        s.cur_kernel = &s.kernels[only];
        std::printf("DROP %s:%d %s SURVIVES (%llu calls dropped)\n", only.c_str(), s.drop_site, hipsim::site_text(s.drop_site).c_str(), s.dropped_calls);
        return 0;
    }
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "ALL OK", failures);
    return failures ? 1 : 0;
}
