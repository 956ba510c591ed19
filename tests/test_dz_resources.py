"""Resource guard for the kernels of include/toyni_hip.h 3o (CPU only: read from the resource remarks of the build that produced the
shipped library, as tests/test_transcript_resources.py does).  DESIGN.md section 8n states the figures: no new kernel uses scratch; the
one-wave preparation kernels use no LDS beyond what they declare (the 64 x 4 words of claim shares in the two DEEP ones, none in the
others) and stay within 128 VGPRs; a device-record instantiation has no more VGPRs than its argument-fed twin plus RECORD_ALLOWANCE,
because the record is read through a read-only pointer argument by scalar loads, exactly as the kernel arguments are: it may cost one
64-bit address held in vector registers and nothing else."""
import re

from test_transcript_resources import _blocks, _of

RECORD_ALLOWANCE = 2
ONE_WAVE = {"transcript_squeeze_ext_point_kernel": 0, "transcript_absorb_fields_kernel": 0, "poly_ext_prepare_kernel": 0,
            "deep_ext_prepare_inline_kernel": 4 * 64 * 4, "deep_ext_prepare_kernel": 4 * 64 * 4}
TWINS = {"poly_eval_ext_batch_partial_dz_kernel": "poly_eval_ext_batch_partial_kernel", "poly_eval_ext_batch_final_dz_kernel": "poly_eval_ext_batch_final_kernel",
         "deep_combine_ext_dz_kernel": "deep_combine_ext_kernel"}


def _one(blocks, kernel):
    found = _of(blocks, kernel)
    assert len(found) == 1, (kernel, sorted(found))
    return next(iter(found.items()))


def test_no_new_kernel_uses_scratch_and_the_preparation_kernels_use_the_lds_they_declare():
    blocks = _blocks()
    for kernel, lds in list(ONE_WAVE.items()) + [("query_rows_kernel", 0)]:
        name, r = _one(blocks, kernel)
        print(name, r)
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        assert r["lds"] == lds and r["vgprs"] <= 128, (name, r)


def test_the_device_record_twins_cost_no_more_registers_than_the_argument_fed_kernels():
    blocks = _blocks()
    for dz, twin in TWINS.items():
        (name, r), (tname, t) = _one(blocks, dz), _one(blocks, twin)
        print(name, r, tname, t)
        assert r["scratch"] == 0 and t["scratch"] == 0, (name, r)
        assert r["lds"] == t["lds"] and r["occupancy"] >= t["occupancy"], (name, r, t)
        assert r["vgprs"] <= t["vgprs"] + RECORD_ALLOWANCE, (name, r["vgprs"], t["vgprs"])
    assert re.search(r"\d+deep_combine_ext_inline_kernel", "\n".join(blocks)), "the inline twin is still there"
