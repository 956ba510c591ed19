"""The C++ packer of toyni_amd/csrc/host/fib_verifier.hpp (toyni::fib::pack_proof) as a stand-alone host program built with
-fsanitize=address,undefined and run as a plain program: a Proof with short, long and empty opening_records / fri_commitments /
fri_final_layer / query_indices is refused by the reference's name without a byte read out of bounds, and a well-formed Proof yields
the image toyni_amd.verifier.pack_fib_proof yields.  Host code only; nothing here is loaded into the interpreter."""
import os
import subprocess

import numpy as np

import __graft_entry__ as entry
import fib_verify_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <cstdio>
#include "%(root)s/toyni_amd/csrc/host/fib_verifier.hpp"
using namespace toyni::fib;
static int failures = 0;
static void expect(const char* what, const Proof& p, const toyni_fib_proof_layout& l, const char* name) {
    std::vector<uint8_t> image(l.image_bytes, 0xA5);
    const std::string got = pack_proof(p, l, image.data());
    bool untouched = true;
    for (uint8_t b : image) untouched = untouched && b == 0xA5;
    if (got != name || !untouched) { ++failures; std::printf("FAIL %%s: \"%%s\", want \"%%s\"%%s\n", what, got.c_str(), name, untouched ? "" : ", image written"); }
}
int main(int argc, char** argv) {
    toyni_fib_proof_layout l;
    if (toyni_fib_proof_layout_of(8, &l) != 0) return 2;
    Proof good;
    good.trace_len = 8; good.lde_size = 256;
    good.fri_commitments.resize(l.folds + 1);
    good.fri_final_layer.assign(l.final_size, 7);
    good.query_indices.resize(l.queries);
    for (size_t i = 0; i < l.queries; ++i) good.query_indices[i] = (uint32_t)(3 * i);
    size_t want = 0;
    for (size_t g = 0; g < l.ngroups; ++g) want += l.group_records[g] * l.group_record_bytes[g];
    good.opening_records.resize(want);
    for (size_t i = 0; i < want; ++i) good.opening_records[i] = (uint8_t)(i * 131 + 7);
    for (size_t k = 0; k < good.fri_commitments.size(); ++k) good.fri_commitments[k].fill((uint8_t)(k + 1));
    good.trace_commitment.fill(0x11); good.quotient_commitment.fill(0x22);
    good.t_z = 1; good.t_gz = 2; good.t_ggz = 3; good.q_z = 4;
    Proof p;
    p = good; p.lde_size = 512; expect("lde_size", p, l, "lde_size");
    p = good; p.trace_len = 16; expect("trace_len", p, l, "lde_size");
    p = good; p.fri_commitments.pop_back(); expect("commitments short", p, l, "fold_count");
    p = good; p.fri_commitments.emplace_back(); expect("commitments long", p, l, "fold_count");
    p = good; p.fri_commitments.clear(); expect("commitments empty", p, l, "fold_count");
    p = good; p.fri_final_layer.push_back(1); expect("final long", p, l, "final_size");
    p = good; p.fri_final_layer.clear(); expect("final empty", p, l, "final_size");
    p = good; p.query_indices.pop_back(); expect("indices short", p, l, "query_count");
    p = good; p.query_indices.clear(); expect("indices empty", p, l, "query_count");
    p = good; p.opening_records.pop_back(); expect("records short", p, l, "fri_opening_count");
    p = good; p.opening_records.push_back(0); expect("records long", p, l, "fri_opening_count");
    p = good; p.opening_records.clear(); p.opening_records.shrink_to_fit(); expect("records empty", p, l, "fri_opening_count");
    std::vector<uint8_t> image(l.image_bytes, 0xA5);
    if (pack_proof(good, l, image.data()) != "") { ++failures; std::printf("FAIL the well-formed proof was refused\n"); }
    if (argc > 1) { FILE* f = std::fopen(argv[1], "wb"); std::fwrite(image.data(), 1, image.size(), f); std::fclose(f); }
    std::printf("%%s (%%d failures)\n", failures ? "FAILED" : "ALL OK", failures);
    return failures ? 1 : 0;
}
'''


def test_the_packer_refuses_by_name_without_reading_out_of_bounds(tmp_path):
    entry.build_hip()
    src, exe, img = tmp_path / "packer.cpp", tmp_path / "packer", tmp_path / "image.bin"
    src.write_text(PROGRAM % {"root": ROOT})
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas",
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L", entry.LIB_DIR, "-ltoyni_hip", f"-Wl,-rpath,{entry.LIB_DIR}",
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    res = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "ALL OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    # the same proof through the Python packer: the same image
    from toyni_amd import verifier
    lay = verifier.fib_proof_layout(8)
    want = sum(lay.group_records[g] * lay.group_record_bytes[g] for g in range(lay.ngroups))
    raw = {"trace_len": 8, "lde_size": 256, "trace_commitment": bytes([0x11]) * 32, "quotient_commitment": bytes([0x22]) * 32, "t_z": 1, "t_gz": 2, "t_ggz": 3,
           "q_z": 4, "fri_commitments": [bytes([k + 1]) * 32 for k in range(lay.folds + 1)], "fri_final_layer": [7] * lay.final_size,
           "query_indices": [3 * i for i in range(44)], "opening_records": ((np.arange(want, dtype=np.uint64) * 131 + 7) & 0xFF).astype(np.uint8)}
    assert verifier.pack_fib_proof(raw) == img.read_bytes()
