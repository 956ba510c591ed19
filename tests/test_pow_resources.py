"""Resource guard for the three kernels of a grind chain (include/toyni_hip.h 3n; CPU only: read from the resource remarks of the build
that produced the shipped library, as tests/test_transcript_resources.py does).  DESIGN.md section 8m states the figures.

The search kernel -- ONE kernel that holds the one-block and the two-block loop, because the length that chooses between them lives in
device memory -- uses no scratch (a message block or a tail template indexed by a run-time word number would show up as such) and no
LDS beyond the shared midstate, eight words.  Its grid is sized for three waves per SIMD (pow_grid_blocks: at most 3 workgroups of
four waves per CU), so the build must admit three.  The two one-wave ends use neither scratch nor LDS.  VGPRs, SGPRs and occupancy are
printed for DESIGN."""
import os
import re

import __graft_entry__ as entry

MIDSTATE_BYTES = 8 * 4


def _blocks():
    entry.build_hip()
    if not os.path.exists(entry.RESOURCES) or os.path.getmtime(entry.RESOURCES) < os.path.getmtime(entry.LIB) - 5:
        entry.build_hip(force=True)
    remarks = open(entry.RESOURCES).read()
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]:
        name = b.split()[0]
        out[name] = {key: int(re.search(pat + r": (\d+)", b).group(1))
                     for key, pat in (("vgprs", "VGPRs"), ("sgprs", "TotalSGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"),
                                      ("lds", r"LDS Size \[bytes/block\]"), ("occupancy", r"Occupancy \[waves/SIMD\]"),
                                      ("vgpr_spill", "VGPRs Spill"))}
    return out


def _of(blocks, kernel):
    return {n: r for n, r in blocks.items() if re.search(r"\d+" + kernel + r"(?![a-z_])", n)}


def test_the_search_kernel_uses_no_scratch_and_no_lds_beyond_the_midstate():
    found = _of(_blocks(), "pow_search_kernel")
    assert len(found) == 1, sorted(found)                  # one symbol: both loops live in it
    for name, r in found.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        assert r["lds"] == MIDSTATE_BYTES, (name, r)
        assert r["occupancy"] >= 3, (name, r)              # the grid of pow_grid_blocks is resident at once


def test_the_ends_of_the_chain_are_plain_one_wave_kernels():
    blocks = _blocks()
    for kernel in ("pow_arm_kernel", "pow_finish_kernel"):
        found = _of(blocks, kernel)
        assert len(found) == 1, (kernel, sorted(found))
        for name, r in found.items():
            print(name, r)
            assert r["scratch"] == 0 and r["lds"] == 0 and r["vgprs"] <= 128, (name, r)
