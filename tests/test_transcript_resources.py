"""Resource guard for the kernels of the device transcript and of the commit phases on it (include/toyni_hip.h 3l; CPU only: read from
the resource remarks of the build that produced the shipped library, as tests/test_rows_resources.py does).  DESIGN.md section 8k states
the figures: no kernel uses scratch (a message block or a register array indexed by a rolled loop would show up as such); the one-wave
kernels stay within 128 VGPRs; the fused rounds, one workgroup of eight waves, within the 256 that two waves per SIMD leave, with an
LDS footprint of exactly the layer, the level, four schedule areas, the transcript and beta."""
import os
import re

import __graft_entry__ as entry

# kernel -> (instantiations, VGPR budget, LDS bytes per instantiation in the order of the mangled names, or None = any of the listed)
ONE_WAVE = {"transcript_absorb_kernel": 0, "transcript_squeeze_kernel": 0, "transcript_squeeze_indices_kernel": 4 * 256 + 4,
            "fri_transcript_round_kernel": 16}
FOLDS = {"fri_fold_commit_rec_kernel": 1, "fri_fold_ext_commit_rec_kernel": 2}
SCHED = 4 * 48 * 64 * 4                                                # four main / helper pairs
TAIL_LDS = {"ILb0E": 2 * 512 * 4 + 512 * 32 + SCHED + 1024 + 16,       # base: the layer of 1024 words
            "ILb1E": 2 * 512 * 16 + 512 * 32 + SCHED + 1024 + 16}      # Ext: 1024 elements of four words


def _blocks():
    entry.build_hip()
    if not os.path.exists(entry.RESOURCES) or os.path.getmtime(entry.RESOURCES) < os.path.getmtime(entry.LIB) - 5:
        entry.build_hip(force=True)
    remarks = open(entry.RESOURCES).read()
    assert "loop not unrolled" not in remarks
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]:
        name = b.split()[0]
        out[name] = {key: int(re.search(pat + r": (\d+)", b).group(1))
                     for key, pat in (("vgprs", "VGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"), ("lds", r"LDS Size \[bytes/block\]"),
                                      ("occupancy", r"Occupancy \[waves/SIMD\]"))}
    return out


def _of(blocks, kernel):
    return {n: r for n, r in blocks.items() if re.search(r"\d+" + kernel + r"(?![a-z_])", n)}


def test_no_new_kernel_uses_scratch_and_the_one_wave_kernels_fit_128_vgprs():
    blocks = _blocks()
    for kernel, lds in ONE_WAVE.items():
        found = _of(blocks, kernel)
        assert len(found) == 1, (kernel, sorted(found))
        for name, r in found.items():
            print(name, r)
            assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
            assert r["vgprs"] <= 128 and r["lds"] == lds, (name, r)
    for kernel, count in list(FOLDS.items()) + [("fri_query_positions_kernel", 1)]:
        found = _of(blocks, kernel)
        assert len(found) == count, (kernel, sorted(found))
        for name, r in found.items():
            print(name, r)
            assert r["scratch"] == 0 and r["lds"] == 0 and r["vgprs"] <= 128, (name, r)
    ext = _of(blocks, "fri_fold_ext_commit_rec_kernel")
    assert any("ILb1E" in n for n in ext) and any("ILb0E" in n for n in ext), sorted(ext)


def test_the_fused_rounds_fit_two_waves_per_simd_and_their_lds_is_what_the_design_states():
    found = _of(_blocks(), "fri_tail_rounds_kernel")
    assert len(found) == 2, sorted(found)
    for name, r in found.items():
        print(name, r)
        tag = "ILb1E" if "ILb1E" in name else "ILb0E"
        assert tag in name
        assert r["scratch"] == 0, f"{name} uses {r['scratch']} bytes of scratch per lane"
        assert r["vgprs"] <= 256 and r["occupancy"] >= 2, (name, r)          # 512 threads = 8 waves = 2 per SIMD
        assert r["lds"] == TAIL_LDS[tag] and r["lds"] <= 160 << 10, (name, r, TAIL_LDS[tag])
