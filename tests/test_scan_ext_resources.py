"""The Ext accumulator-column kernels (include/toyni_hip.h 3i) keep a thread's group of Ext elements -- 16 words of terms, 16 of running
values -- in registers that are indexed by constants only: none of the four kernel families may use scratch (CPU only: read from the
resource record of the build that produced the shipped library, as tests/test_scan_resources.py does)."""
import os
import re

import __graft_entry__ as entry


def test_no_ext_accumulator_kernel_uses_scratch():
    entry.build_hip()
    if not os.path.exists(entry.RESOURCES) or os.path.getmtime(entry.RESOURCES) < os.path.getmtime(entry.LIB) - 5:
        entry.build_hip(force=True)
    remarks = open(entry.RESOURCES).read()
    blocks = re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]
    seen = set()
    for b in blocks:
        name = b.split(" ")[0]
        if "ext_accum" not in name and "ext_invert" not in name:
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
        assert m, name
        assert int(m.group(1)) == 0, f"{name} uses {m.group(1)} bytes of scratch per lane"
        seen.add(name)
    # aggregate, prefix and apply for each op, and the inversion
    families = ("ext_accum_aggregate_kernel", "ext_accum_prefix_kernel", "ext_accum_apply_kernel")
    assert len(seen) == 7 and all(sum(f in s for s in seen) == 2 for f in families) and sum("ext_invert_columns_kernel" in s for s in seen) == 1, sorted(seen)
