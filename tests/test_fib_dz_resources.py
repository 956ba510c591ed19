"""Resource guard for the kernels of include/toyni_hip.h 3q (CPU only: read from the resource remarks of the build that produced the
shipped library, as tests/test_dc_resources.py does).  In this build each record-fed twin has exactly the VGPRs, the LDS and the
occupancy of its argument-fed original and no scratch: the record is read through a read-only pointer argument by scalar loads, as
the kernel arguments are.  No new kernel uses scratch (the mask selects its keystream words with constant register indices), and the
one-wave kernels use no LDS.  The three originals are what the parent commit's build made them: VGPRs, SGPRs, LDS and occupancy
below are read from that build's remarks."""
from test_dc_resources import _one, _sgprs
from test_transcript_resources import _blocks

NEW = ["fib_mask_kernel", "transcript_squeeze_point_kernel", "poly_dz_prepare_kernel", "poly_eval_partial_dz_kernel", "poly_eval_final_dz_kernel",
       "fib_deep_prepare_kernel", "fib_deep_dz_kernel", "fri_phase_roots_kernel"]
ONE_WAVE = ["transcript_squeeze_point_kernel", "poly_dz_prepare_kernel", "fib_deep_prepare_kernel"]
TWINS = {r"\d+fib_deep_dz_kernelN": r"\d+fib_deep_kernelN", r"\d+poly_eval_partial_dz_kernelN": r"\d+poly_eval_partial_kernelN",
         r"\d+poly_eval_final_dz_kernelN": r"\d+poly_eval_final_kernelN"}
# the parent build: original -> (VGPRs, SGPRs, LDS bytes, waves per SIMD), none with scratch
PARENT = {r"\d+fib_deep_kernelN": (60, 68, 0, 8), r"\d+poly_eval_partial_kernelN": (26, 44, 1024, 8), r"\d+poly_eval_final_kernelN": (14, 54, 1024, 8)}


def test_no_new_kernel_uses_scratch_and_the_one_wave_kernels_use_no_lds():
    blocks = _blocks()
    for kernel in NEW:
        name, r = _one(blocks, r"\d+" + kernel + r"(?![a-z_])")
        print(name, r)
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        if kernel in ONE_WAVE:
            assert r["lds"] == 0 and r["vgprs"] <= 128, (name, r)


def test_each_twin_has_the_registers_lds_and_occupancy_of_its_original():
    blocks = _blocks()
    for twin, original in TWINS.items():
        (name, r), (oname, o) = _one(blocks, twin), _one(blocks, original)
        print(name, r, oname, o)
        assert r["scratch"] == 0 and o["scratch"] == 0, (name, r)
        assert (r["vgprs"], r["lds"], r["occupancy"]) == (o["vgprs"], o["lds"], o["occupancy"]), (name, r, o)


def test_the_argument_fed_originals_are_what_the_parent_build_made_them():
    blocks, sgprs = _blocks(), _sgprs()
    for pattern, (vgprs, sg, lds, occupancy) in PARENT.items():
        name, r = _one(blocks, pattern)
        print(name, r, sgprs[name])
        assert (r["vgprs"], sgprs[name], r["lds"], r["occupancy"], r["scratch"]) == (vgprs, sg, lds, occupancy, 0), (name, r, sgprs[name])
