"""Resource guard for the Ext fold-and-commit kernel (CPU only: read from the resource remarks of the build that produced the shipped
library, as tests/test_rows_resources.py does).  The folded element goes from registers into the leaf hash; a byte buffer or a
register array indexed by a rolled loop would show up here as scratch.  VGPRs and occupancy are printed, not bounded."""
import os
import re

import __graft_entry__ as entry

KERNEL = "fri_fold_ext_commit_kernel"


def test_fold_ext_commit_kernel_has_both_instantiations_and_no_scratch():
    entry.build_hip()
    if not os.path.exists(entry.RESOURCES) or os.path.getmtime(entry.RESOURCES) < os.path.getmtime(entry.LIB) - 5:
        entry.build_hip(force=True)
    remarks = open(entry.RESOURCES).read()
    assert "loop not unrolled" not in remarks
    blocks = re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        if KERNEL not in name:
            continue

        def field(key):
            m = re.search(key + r": (\d+)", b)
            assert m, (name, key)
            return int(m.group(1))

        scratch = field(r"ScratchSize \[bytes/lane\]")
        print(f"{name}: VGPRs {field('VGPRs')}, SGPRs {field('SGPRs')}, occupancy {field(r'Occupancy .waves/SIMD.')} waves/SIMD, "
              f"scratch {scratch} B/lane")
        assert scratch == 0, f"{name} uses {scratch} bytes of scratch per lane"
        assert field(r"LDS Size \[bytes/block\]") == 0, name          # no shared memory: nothing for a barrier to guard
        seen[name] = True
    # SALTED = true and false (Itanium mangling: ILb1EE / ILb0EE)
    assert len(seen) == 2 and any("ILb1E" in n for n in seen) and any("ILb0E" in n for n in seen), sorted(seen)
