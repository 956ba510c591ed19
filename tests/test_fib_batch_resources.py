"""The batch twins of include/toyni_hip.h 3s are written out, as 3r's were, and live in a translation unit of their own
(toyni_amd/csrc/batch/toyni_hip_fib_batch.hip, linked into libtoyni_hip.so), so that the existing kernels' code cannot move and the build of
toyni_hip.hip keeps its kernel list.  This file holds the build to that: toyni_hip.hip yields exactly the kernels of the parent build,
each with its resource lines; the new unit yields the thirteen kernels of 3s and nothing else; none of them uses scratch, the one-wave
kernels use no LDS, and each twin equals its original in VGPRs, LDS and occupancy.

PARENT is the parent commit's toyni_amd/lib/libtoyni_hip.resources.txt reduced by tests/test_batch_resources._parse: the table of that
file (the build before 3r; this build still has every line of it) and, below, the thirteen symbols 3r added, printed from the parent
build in the same way.  CPU only."""
import test_batch_resources as base
from test_batch_resources import FIELDS, _kernel_of

TWINS = {"chacha20_fill_batch_kernel": "chacha20_fill_kernel", "fib_mask_batch_kernel": "fib_mask_kernel",
         "fib_quotient_batch_kernel": "fib_quotient_kernel", "transcript_squeeze_point_batch_kernel": "transcript_squeeze_point_kernel",
         "transcript_absorb_fields_batch_kernel": "transcript_absorb_fields_kernel", "poly_dz_prepare_batch_kernel": "poly_dz_prepare_kernel",
         "poly_eval_partial_dz_batch_kernel": "poly_eval_partial_dz_kernel", "poly_eval_final_dz_batch_kernel": "poly_eval_final_dz_kernel",
         "fib_deep_prepare_batch_kernel": "fib_deep_prepare_kernel", "fib_deep_dz_batch_kernel": "fib_deep_dz_kernel",
         "query_rows_batch_kernel": "query_rows_kernel", "fri_phase_roots_batch_kernel": "fri_phase_roots_kernel"}
NEW = set(TWINS) | {"copy_rows_kernel"}          # copy_rows_kernel has no twin
ONE_WAVE = {"transcript_squeeze_point_batch_kernel", "transcript_absorb_fields_batch_kernel", "poly_dz_prepare_batch_kernel",
            "fib_deep_prepare_batch_kernel", "fri_phase_roots_batch_kernel"}

PARENT_3R = {
    "_Z24merkle_leaf_batch_kernelPKjmPKhmPhmm": (95, 91, 0, 0, 5, 0, 0, 0),
    "_Z25merkle_level_batch_kernelPhmmmm": (97, 94, 0, 0, 5, 0, 0, 0),
    "_Z30merkle_level_coop_batch_kernelPhmmmm": (32, 122, 0, 0, 4, 0, 0, 12288),
    "_Z24merkle_tail_batch_kernelPhmmj": (62, 127, 0, 0, 4, 0, 0, 65536),
    "_Z30transcript_absorb_batch_kernelPN5toyni15TranscriptStateEPKhmj": (29, 38, 0, 0, 8, 0, 0, 0),
    "_Z39transcript_squeeze_indices_batch_kernelPN5toyni15TranscriptStateEjjPjm": (52, 104, 0, 0, 4, 0, 0, 1028),
    "_Z32fri_query_positions_batch_kernelPKjmjmmPjm": (32, 17, 0, 0, 8, 0, 0, 0),
    "_Z33fri_transcript_round_batch_kernelPN5toyni15TranscriptStateEPKhmjjjPjjS4_m": (56, 101, 0, 0, 4, 0, 0, 16),
    "_Z32fri_fold_commit_rec_batch_kernelN5toyni8FoldArgsE9FoldBatchPKjPKhPh": (106, 92, 0, 0, 5, 0, 0, 0),
    "_Z36fri_fold_ext_commit_rec_batch_kernelILb1EEvN5toyni8FoldArgsE9FoldBatchPKjPKhPh": (106, 89, 0, 0, 5, 0, 0, 0),
    "_Z36fri_fold_ext_commit_rec_batch_kernelILb0EEvN5toyni8FoldArgsE9FoldBatchPKjPKhPh": (106, 86, 0, 0, 5, 0, 0, 0),
    "_Z28fri_tail_rounds_batch_kernelILb1EEv11FriTailArgs12FriTailBatch": (106, 157, 0, 0, 2, 8, 0, 82960),
    "_Z28fri_tail_rounds_batch_kernelILb0EEv11FriTailArgs12FriTailBatch": (106, 150, 0, 0, 3, 8, 0, 70672),
}
PARENT = dict(base.PARENT, **PARENT_3R)


def _build_new():
    base.entry.build_hip()
    return base._parse(base.entry.RESOURCES_FIB_BATCH)


def test_every_kernel_of_the_parent_build_keeps_its_resource_lines_and_the_new_unit_holds_the_new_kernels():
    now = base._build()
    assert len(PARENT) == len(base.PARENT) + 13
    gone = sorted(k for k in PARENT if k not in now)
    assert not gone, gone
    moved = {k: (PARENT[k], now[k]) for k in PARENT if now[k] != PARENT[k]}
    assert not moved, "\n".join("%s: %s\n  parent %r\n  now    %r" % (k, FIELDS, a, b) for k, (a, b) in moved.items())
    assert sorted(k for k in now if k not in PARENT) == []                      # toyni_hip.hip: the parent's kernels, no others
    new = sorted(_build_new())
    assert len(new) == len(NEW) and {_kernel_of(k) for k in new} == NEW and not set(new) & set(now), new


def test_the_new_kernels_need_no_scratch_and_the_twins_equal_their_originals():
    at = {f: FIELDS.index(f) for f in FIELDS}
    seen = 0
    for k, v in _build_new().items():
        seen += 1
        name = _kernel_of(k)
        assert v[at["ScratchSize [bytes/lane]"]] == 0 and v[at["VGPRs Spill"]] == 0 and v[at["SGPRs Spill"]] == 0, (k, v)
        if name in ONE_WAVE:
            assert v[at["LDS Size [bytes/block]"]] == 0, (k, v)
        if name not in TWINS:
            continue
        originals = [o for o in PARENT if _kernel_of(o) == TWINS[name]]
        assert len(originals) == 1, (k, originals)
        orig = PARENT[originals[0]]
        for f in ("VGPRs", "AGPRs", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"):
            assert v[at[f]] == orig[at[f]], (k, f, v, orig)
    assert seen == len(NEW)
