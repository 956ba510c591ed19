"""Resource guard for the four-to-one Ext fold-and-commit kernels (CPU only: read from the resource remarks of the build that produced
the shipped library, as tests/test_fold_ext_commit_resources.py does).  A thread holds 16 input elements (64 words), then 16 folded
words that go from registers into three compressions; a byte buffer, or the chunk loader indexing the folded words by a loop
variable, would show up here as scratch.  No LDS: nothing for a barrier to guard.  VGPRs and occupancy are printed, not bounded."""
import os
import re

import __graft_entry__ as entry

KERNELS = ("fri_fold4_ext_commit_kernel", "fri_fold4_ext_commit_rec_kernel")


def test_both_fold4_kernels_have_both_instantiations_no_scratch_and_no_lds():
    entry.build_hip()
    if not os.path.exists(entry.RESOURCES) or os.path.getmtime(entry.RESOURCES) < os.path.getmtime(entry.LIB) - 5:
        entry.build_hip(force=True)
    remarks = open(entry.RESOURCES).read()
    assert "loop not unrolled" not in remarks
    blocks = re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]
    seen = {k: {} for k in KERNELS}
    for b in blocks:
        name = b.split()[0]
        kernel = next((k for k in KERNELS if re.search(r"\d+" + k + "I", name)), None)     # the mangled name: <length><name>I<args>E
        if kernel is None:
            continue

        def field(key):
            m = re.search(key + r": (\d+)", b)
            assert m, (name, key)
            return int(m.group(1))

        scratch = field(r"ScratchSize \[bytes/lane\]")
        print(f"{name}: VGPRs {field('VGPRs')}, SGPRs {field('SGPRs')}, occupancy {field(r'Occupancy .waves/SIMD.')} waves/SIMD, "
              f"scratch {scratch} B/lane")
        assert scratch == 0, f"{name} uses {scratch} bytes of scratch per lane"
        assert field(r"LDS Size \[bytes/block\]") == 0, name
        seen[kernel][name] = True
    for kernel, names in seen.items():      # SALTED = true and false (Itanium mangling: ILb1EE / ILb0EE)
        assert len(names) == 2 and any("ILb1E" in n for n in names) and any("ILb0E" in n for n in names), (kernel, sorted(names))
