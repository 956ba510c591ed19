"""The kernels of include/toyni_hip.h 3t live in a translation unit of their own (toyni_amd/csrc/verify/toyni_hip_verify.hip, linked into
libtoyni_hip.so), whose remarks the build keeps beside the library (__graft_entry__.RESOURCES_VERIFY): the unit holds exactly the five
new kernels, none of them has scratch or spills, the one-wave kernels use no LDS -- except the global checks, which use exactly the
516 bytes the header states (sixteen digests of the final layer's tree and the one word of any_lane) -- and the new symbols are in
neither of the two existing units (whose own lists tests/test_batch_resources.py and tests/test_fib_batch_resources.py hold).
CPU only."""
import re
import subprocess

import test_batch_resources as base
from test_batch_resources import FIELDS, _kernel_of

NEW = {"fib_verify_replay_kernel", "fib_verify_global_kernel", "merkle_verify_records_batch_kernel", "fib_verify_query_kernel", "fib_verify_verdict_kernel"}
ONE_WAVE_LDS = {"fib_verify_replay_kernel": 0, "fib_verify_global_kernel": 516, "fib_verify_query_kernel": 0, "fib_verify_verdict_kernel": 0}


def _build_new():
    base.entry.build_hip()
    return base._parse(base.entry.RESOURCES_VERIFY)


def test_the_third_unit_holds_exactly_the_new_kernels_and_they_are_in_no_other_unit():
    new = _build_new()
    assert len(new) == len(NEW) and {_kernel_of(k) for k in new} == NEW, sorted(new)
    others = set(base._build()) | set(base._parse(base.entry.RESOURCES_FIB_BATCH))
    assert not set(new) & others and not {_kernel_of(k) for k in others} & NEW
    syms = subprocess.run(["nm", "-D", "--defined-only", base.entry.LIB], capture_output=True, text=True).stdout
    assert all(re.search(r"\b%s\b" % re.escape(k), syms) for k in new), [k for k in new if k not in syms]


def test_no_scratch_no_spills_and_the_lds_the_header_states():
    at = {f: FIELDS.index(f) for f in FIELDS}
    seen = 0
    for k, v in _build_new().items():
        seen += 1
        name = _kernel_of(k)
        assert v[at["ScratchSize [bytes/lane]"]] == 0 and v[at["VGPRs Spill"]] == 0 and v[at["SGPRs Spill"]] == 0, (k, v)
        assert v[at["LDS Size [bytes/block]"]] == ONE_WAVE_LDS.get(name, 0), (k, v)
        assert v[at["Occupancy [waves/SIMD]"]] >= 4, (k, v)
    assert seen == len(NEW)
    header = open(base.entry.ROOT + "/include/toyni_hip.h").read()
    assert "516 bytes of LDS" in header
