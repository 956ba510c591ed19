"""Verifying Fibonacci proofs on the device (include/toyni_hip.h 3t): the proof image, its packer and the batch call.

`pack_fib_proof` turns a proof in wire form (the dict of tests/harness and of the compiled provers' JSON: commitments, the four
out-of-domain values, fri_commitments, fri_final_layer, query_indices, opening_records) into the fixed-size image the device reads;
it refuses what the reference verifier refuses on the proof's structure, under the reference's names (an image of the right size
cannot carry those defects).  `verify_fib_batch` uploads the images once, enqueues the chain, downloads 4 x batch bytes once and
synchronises once.  No CPU path: the checks themselves run in csrc/verify/toyni_hip_verify.hip only."""
import ctypes

import numpy as np

from ._lib import c_size, c_void_p, check, lib

NUM_QUERIES, BLOWUP = 44, 32
MAX_GROUPS = 32
CODES = {0: "accept", 1: "malformed", 2: "ood", 3: "final_not_constant", 4: "final_commitment", 5: "query_index", 6: "trace_merkle",
         7: "quotient_merkle", 8: "deep_merkle", 9: "deep_value", 255: "final_value"}


class FibProofLayout(ctypes.Structure):
    """toyni_fib_proof_layout"""
    _fields_ = [(k, c_size) for k in ("trace_len", "lde_size", "folds", "final_size", "queries", "roots_offset", "nroots", "ood_offset",
                                      "indices_offset", "final_offset", "records_offset", "ngroups")] + \
               [(k, c_size * MAX_GROUPS) for k in ("group_offset", "group_leaves", "group_records", "group_record_bytes")] + \
               [("nrecords", c_size), ("image_bytes", c_size)]


class MerkleVerifyGroup(ctypes.Structure):
    """toyni_merkle_verify_group"""
    _fields_ = [("d_records", c_void_p), ("record_stride", c_size), ("nrecords", c_size), ("leaves", c_size), ("salted", ctypes.c_int),
                ("d_indices", c_void_p), ("index_stride", c_size), ("d_root", c_void_p), ("root_stride", c_size), ("d_flags", c_void_p),
                ("flag_stride", c_size)]


class ProofStructureError(ValueError):
    """A proof whose structure the reference verifier refuses; `.name` is the reference's name of the refusal."""

    def __init__(self, name, detail):
        super().__init__(f"{name}: {detail}")
        self.name = name


def fib_proof_layout(trace_len: int) -> FibProofLayout:
    lay = FibProofLayout()
    check(lib.toyni_fib_proof_layout_of(trace_len, ctypes.byref(lay)), "proof layout")
    return lay


def fib_proof_image_bytes(trace_len: int) -> int:
    return lib.toyni_fib_proof_image_bytes(trace_len)


def verdict_string(word: int) -> str:
    return lib.toyni_fib_verdict_string(word).decode()


def decode_verdict(word: int):
    """(word, name, query or None, FRI layer or None)"""
    word = int(word)
    code, q1 = word & 0xFF, word >> 8
    layer = 1 + (code - 16) // 2 if q1 and 16 <= code < 255 else None
    return word, verdict_string(word), (q1 - 1 if q1 else None), layer


def pack_fib_proof(raw) -> bytes:
    """The image of a proof in wire form.  Raises ProofStructureError named lde_size, fold_count, final_size, query_count or
    fri_opening_count (src/verifier.rs: the refusals that precede every cryptographic check)."""
    n = int(raw["trace_len"])
    lay = fib_proof_layout(n)
    if int(raw["lde_size"]) != n * BLOWUP:
        raise ProofStructureError("lde_size", f"{raw['lde_size']} for a trace of {n}")
    roots = [bytes(raw["trace_commitment"]), bytes(raw["quotient_commitment"])] + [bytes(c) for c in raw["fri_commitments"]]
    if len(roots) != lay.nroots or any(len(r) != 32 for r in roots):
        raise ProofStructureError("fold_count", f"{len(roots) - 2} FRI commitments, want {lay.folds + 1} of 32 bytes")
    final = [int(v) for v in raw["fri_final_layer"]]
    if len(final) != lay.final_size:
        raise ProofStructureError("final_size", f"{len(final)} final values, want {lay.final_size}")
    qidx = [int(v) for v in raw["query_indices"]]
    if len(qidx) != NUM_QUERIES:
        raise ProofStructureError("query_count", f"{len(qidx)} queries, want {NUM_QUERIES}")
    records = np.frombuffer(bytes(np.asarray(raw["opening_records"], dtype=np.uint8).tobytes()), dtype=np.uint8)
    want = sum(lay.group_records[g] * lay.group_record_bytes[g] for g in range(lay.ngroups))
    if records.size != want:
        raise ProofStructureError("fri_opening_count", f"{records.size} bytes of opening records, want {want}")
    words = [int(raw[k]) for k in ("t_z", "t_gz", "t_ggz", "q_z")] + qidx + final
    if any(not 0 <= w < 1 << 32 for w in words):
        raise ValueError("a value or index does not fit a 32-bit word")
    img = np.zeros(lay.image_bytes, dtype=np.uint8)
    img[:32 * lay.nroots] = np.frombuffer(b"".join(roots), dtype=np.uint8)
    img[lay.ood_offset:lay.ood_offset + 4 * len(words)] = np.array(words, dtype="<u4").view(np.uint8)
    img[lay.records_offset:lay.records_offset + want] = records
    return img.tobytes()


class _DeviceBytes:
    def __init__(self, nbytes):
        self.ptr = c_void_p()
        check(lib.toyni_malloc(ctypes.byref(self.ptr), max(int(nbytes), 16)), "device allocation failed")

    def free(self):
        if self.ptr:
            lib.toyni_free(self.ptr)
            self.ptr = None


def verify_images(images, trace_len: int, ctx=None, stream: int = 0):
    """images: a list of image byte strings of one trace length.  The verdict words (numpy u32), one per image."""
    from .ntt import NttContext
    lay = fib_proof_layout(trace_len)
    batch = len(images)
    if batch == 0:
        return np.zeros(0, dtype=np.uint32)
    stride = lay.image_bytes
    host = np.zeros(batch * stride, dtype=np.uint8)
    for b, img in enumerate(images):
        if len(img) != lay.image_bytes:
            raise ValueError(f"image {b}: {len(img)} bytes, want {lay.image_bytes}")
        host[b * stride:(b + 1) * stride] = np.frombuffer(img, dtype=np.uint8)
    own = ctx is None
    if own:
        ctx = NttContext(lay.lde_size)
    d_img, d_work, d_out = (_DeviceBytes(host.size), _DeviceBytes(lib.toyni_fib_verify_work_bytes(trace_len, batch)), _DeviceBytes(4 * batch))
    try:
        verdicts = np.zeros(batch, dtype=np.uint32)
        check(lib.toyni_memcpy_h2d_async(d_img.ptr, host.ctypes.data, host.size, stream or None), "image upload failed")
        check(lib.toyni_fib_verify_batch_device(ctx.handle, d_img.ptr, stride, trace_len, batch, d_work.ptr, d_out.ptr, stream or None),
              "GPU proof verification failed")
        check(lib.toyni_memcpy_d2h_async(verdicts.ctypes.data, d_out.ptr, 4 * batch, stream or None), "verdict download failed")
        check(lib.toyni_stream_synchronize(None, stream or None), "stream synchronize failed")
        return verdicts
    finally:
        for d in (d_img, d_work, d_out):
            d.free()
        if own:
            ctx.destroy()


def verify_fib_batch(raws, ctx=None, stream: int = 0):
    """raws: proofs of ONE trace length in wire form.  A list of (word, name, query, layer), one per proof: word 0 / name "accept", or the
    check at which the reference verifier returns false, the query it belongs to (None for the checks made once per proof) and the FRI
    layer (None unless the check is one of a layer)."""
    raws = list(raws)
    if not raws:
        return []
    n = int(raws[0]["trace_len"])
    if any(int(r["trace_len"]) != n for r in raws):
        raise ValueError("the proofs of a batch have one trace length")
    return [decode_verdict(w) for w in verify_images([pack_fib_proof(r) for r in raws], n, ctx=ctx, stream=stream)]
