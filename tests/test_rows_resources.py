"""Resource guard for the row-leaf Merkle kernels (CPU only: read from the resource remarks of the build that produced the shipped
library, as tests/test_build_resources.py does).  The leaf hash streams its message through registers block by block; a byte buffer
or a register array indexed by a rolled loop would show up here as scratch.  VGPRs and occupancy are printed, not bounded."""
import os
import re

import __graft_entry__ as entry

ROW_KERNELS = ("merkle_rows_leaf_kernel", "merkle_open_rows_kernel")


def test_row_kernels_have_no_scratch_and_no_rolled_register_loops():
    entry.build_hip()
    if not os.path.exists(entry.RESOURCES) or os.path.getmtime(entry.RESOURCES) < os.path.getmtime(entry.LIB) - 5:
        entry.build_hip(force=True)
    remarks = open(entry.RESOURCES).read()
    # "loop not unrolled" warnings name the source line, not the kernel: none may point into the row-leaf code (the translation unit as a
    # whole is held to zero of them by tests/test_build_resources.py)
    for line in remarks.split("\n"):
        if "loop not unrolled" in line:
            assert "merkle_kernels.hpp" not in line and "merkle_rows" not in line and "merkle_open_rows" not in line, line
    assert "loop not unrolled" not in remarks
    blocks = re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        if not any(k in name for k in ROW_KERNELS):
            continue

        def field(key):
            m = re.search(key + r": (\d+)", b)
            assert m, (name, key)
            return int(m.group(1))

        scratch = field(r"ScratchSize \[bytes/lane\]")
        print(f"{name}: VGPRs {field('VGPRs')}, SGPRs {field('SGPRs')}, occupancy {field(r'Occupancy .waves/SIMD.')} waves/SIMD, "
              f"scratch {scratch} B/lane")
        assert scratch == 0, f"{name} uses {scratch} bytes of scratch per lane"
        seen[name] = True
    # layout x salted leaf kernels, one opening kernel
    assert sum("merkle_rows_leaf_kernel" in n for n in seen) == 4, sorted(seen)
    assert sum("merkle_open_rows_kernel" in n for n in seen) == 1, sorted(seen)
