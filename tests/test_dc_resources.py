"""Resource guard for the kernels of include/toyni_hip.h 3p (CPU only: read from the resource remarks of the build that produced the
shipped library, as tests/test_dz_resources.py does).  DESIGN.md section 8o states the figures: no new kernel uses scratch; the two
one-wave preparation kernels use no LDS (no lane reads what another wrote) and stay within 128 VGPRs; a record-fed twin has the LDS
and at least the occupancy of its argument-fed original and no more VGPRs than it plus RECORD_ALLOWANCE -- the allowance and the reason
of tests/test_dz_resources.py: the record is read through a read-only pointer argument by scalar loads, exactly as the kernel
arguments are, so it may cost one 64-bit address held in vector registers and nothing else.  And the argument-fed originals, whose
source was moved into bodies that the twins share, are what the parent commit's build made them: VGPRs, SGPRs, LDS and occupancy as
section 8o quotes them from that build."""
import re

from test_transcript_resources import _blocks

RECORD_ALLOWANCE = 2
ONE_WAVE = ["air_dc_prepare_kernel", "extcol_dc_prepare_kernel"]
# twin -> original, as regular expressions on the mangled names (ILi0E: the sum, ILi1E: the product)
TWINS = {r"\d+air_quotient_ext_dc_kernelN": r"\d+air_quotient_ext_kernelN",
         r"\d+extcol_aggregate_dc_kernelILi0E": r"\d+ext_accum_aggregate_kernelILi0E", r"\d+extcol_aggregate_dc_kernelILi1E": r"\d+ext_accum_aggregate_kernelILi1E",
         r"\d+extcol_apply_dc_kernelILi0E": r"\d+ext_accum_apply_kernelILi0E", r"\d+extcol_apply_dc_kernelILi1E": r"\d+ext_accum_apply_kernelILi1E"}
# the parent build: original -> (VGPRs, SGPRs, LDS bytes, waves per SIMD), none with scratch
PARENT = {r"\d+air_quotient_ext_kernelN": (76, 46, 0, 6), r"\d+air_quotient_ext_inline_kernelN": (76, 46, 0, 6),
          r"\d+ext_accum_aggregate_kernelILi0E": (68, 58, 80, 7), r"\d+ext_accum_aggregate_kernelILi1E": (58, 58, 80, 8),
          r"\d+ext_accum_prefix_kernelILi0E": (50, 78, 80, 8), r"\d+ext_accum_prefix_kernelILi1E": (43, 89, 80, 8),
          r"\d+ext_accum_apply_kernelILi0E": (68, 60, 80, 7), r"\d+ext_accum_apply_kernelILi1E": (58, 65, 80, 8)}


def _one(blocks, pattern):
    found = {n: r for n, r in blocks.items() if re.search(pattern, n)}
    assert len(found) == 1, (pattern, sorted(found))
    return next(iter(found.items()))


def _sgprs():
    import __graft_entry__ as entry
    remarks = open(entry.RESOURCES).read()
    return {b.split()[0]: int(re.search(r"TotalSGPRs: (\d+)", b).group(1)) for b in re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]}


def test_no_new_kernel_uses_scratch_and_the_preparation_kernels_use_no_lds():
    blocks = _blocks()
    for kernel in ONE_WAVE:
        name, r = _one(blocks, r"\d+" + kernel + r"(?![a-z_])")
        print(name, r)
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        assert r["lds"] == 0 and r["vgprs"] <= 128, (name, r)


def test_the_record_fed_twins_cost_no_more_registers_than_the_argument_fed_kernels():
    blocks = _blocks()
    for twin, original in TWINS.items():
        (name, r), (oname, o) = _one(blocks, twin), _one(blocks, original)
        print(name, r, oname, o)
        assert r["scratch"] == 0 and o["scratch"] == 0, (name, r)
        assert r["lds"] == o["lds"] and r["occupancy"] >= o["occupancy"], (name, r, o)
        assert r["vgprs"] <= o["vgprs"] + RECORD_ALLOWANCE, (name, r["vgprs"], o["vgprs"])


def test_the_argument_fed_originals_are_what_the_parent_build_made_them():
    blocks, sgprs = _blocks(), _sgprs()
    for pattern, (vgprs, sg, lds, occupancy) in PARENT.items():
        name, r = _one(blocks, pattern)
        print(name, r, sgprs[name])
        assert (r["vgprs"], sgprs[name], r["lds"], r["occupancy"], r["scratch"]) == (vgprs, sg, lds, occupancy, 0), (name, r, sgprs[name])
