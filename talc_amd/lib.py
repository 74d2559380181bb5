"""ctypes binding of libtalc_hip.so (include/talc_hip.h) — the product's C ABI.

There is no CPU fallback: every compute entry point needs a MI355X and fails loudly
(TalcError) without one.  Loading the library and resolving its symbols works on any host.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import build as _build

_LIB = None

READ_CORRECTED, READ_SKIPPED_SHORT, READ_NO_SOLID_KMER, READ_NO_STRUCTURE, READ_ERROR = range(5)
LOG_MESSAGES = {
    READ_NO_SOLID_KMER: "No solid kmer could be found.",          # main.cpp:294
    READ_NO_STRUCTURE: "Unable to define convenient structure.",  # main.cpp:290
}

SEG_SOLID, SEG_CORRECTED, SEG_RAW = range(3)
SEG_LETTERS = "SCR"
# talc_segment (docs/correction_map.md)
SEGMENT_DTYPE = np.dtype([("kind", "<u4"), ("raw_start", "<u4"), ("raw_len", "<u4"), ("out_start", "<u4"), ("out_len", "<u4")])
# talc_solidity (docs/solidity.md)
SOLIDITY_FIELDS = ("n_kmers", "n_solid", "n_in", "n_regions", "solid_bases", "longest_weak")
SOLIDITY_DTYPE = np.dtype([(f, "<u4") for f in SOLIDITY_FIELDS])
# talc_piece_mode, talc_piece (docs/trim_split.md)
PIECES_TRIM, PIECES_SPLIT = 1, 2
PIECE_DTYPE = np.dtype([("read", "<u4"), ("out_start", "<u4"), ("out_len", "<u4")])
# talc_edit_row and the op codes (docs/correction_edits.md): an op is len << 4 | code, the codes are BAM's
EDIT_ROW_FIELDS = ("n_match", "n_mismatch", "n_ins", "n_del", "n_ops", "n_unaligned")
EDIT_ROW_DTYPE = np.dtype([(f, "<u4") for f in EDIT_ROW_FIELDS])
EDIT_I, EDIT_D, EDIT_EQ, EDIT_X = 1, 2, 7, 8
# talc_strand (docs/auto_strand.md)
STRAND_FIELDS = ("n_kmers", "fwd_solid", "fwd_in", "rc_solid", "rc_in", "reverse")
STRAND_DTYPE = np.dtype([(f, "<u4") for f in STRAND_FIELDS])
# talc_end_row (docs/read_ends.md)
ENDS_DTYPE = np.dtype([("head_adapter_len", "<u4"), ("head_poly_len", "<u4"), ("tail_adapter_len", "<u4"), ("tail_poly_len", "<u4"),
                       ("head_adapter", "u1"), ("head_adapter_err", "u1"), ("tail_adapter", "u1"), ("tail_adapter_err", "u1"),
                       ("kept_start", "<u4"), ("kept_len", "<u4"), ("orient", "<i4")])
# talc_chimera_hit, talc_split_piece (docs/chimeras.md)
CHIMERA_DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("end", "<u4"), ("adapter", "u1"), ("strand", "u1"), ("err", "u1"), ("pad", "u1")])
SPLIT_PIECE_DTYPE = np.dtype([("read", "<u4"), ("start", "<u4"), ("len", "<u4"), ("ordinal", "<u4")])
# how k_read_chimera walks a read (talc_chimera_plan.h: chimera_geometry), for tests that aim at its borders
CHIMERA_CHUNK_MIN, CHIMERA_CHUNK_MAX = 36, 252


def chimera_geometry(length, n_patterns):
    """(lanes per pattern, chunk, tile) of a read of `length` bytes under n_patterns = 2 * adapters patterns: lane q of a
    pattern owns columns [tile_start + q * chunk, + chunk) of every tile."""
    lanes = 64 // n_patterns
    chunk = min(CHIMERA_CHUNK_MAX, max(CHIMERA_CHUNK_MIN, -(-length // lanes)))
    chunk += (4 - chunk % 8) % 8
    return lanes, chunk, lanes * chunk
# talc_demux_row and its status codes (docs/demux.md)
DEMUX_DTYPE = np.dtype([("barcode", "u1"), ("status", "u1"), ("head_best", "u1"), ("head_err", "u1"), ("head_margin", "u1"),
                        ("tail_best", "u1"), ("tail_err", "u1"), ("tail_margin", "u1"), ("head_end", "<u4"), ("tail_end", "<u4")])
DEMUX_NONE, DEMUX_BOTH, DEMUX_HEAD_ONLY, DEMUX_TAIL_ONLY, DEMUX_CONFLICT = range(5)
DEMUX_MAX_BARCODES, DEMUX_DEFAULT_WINDOW = 96, 256
# the defaults of the command line and of Context.set_demux (docs/demux.md, "Why 20 per cent and a margin of 2")
DEMUX_DEFAULT_ERR, DEMUX_DEFAULT_MARGIN = 20, 2


def demux_geometry(n_barcodes, window=DEMUX_DEFAULT_WINDOW):
    """How k_read_demux deals its 2 * n_barcodes patterns (end, barcode) over the lanes of its wave (talc_kernels_demux.h:
    demux_geometry), for tests that aim at its borders: (chunks, passes, tail_slot, chunk).  A slot is lane + 64 * pass.
    Up to 16 barcodes: one pass, every pattern gets `chunks` lanes, each `chunk` columns of a text of `window` columns behind
    a warm-up; pattern (end, b) starts at slot (end * n_barcodes + b) * chunks.  From 17 on: chunks is 1, the head of barcode
    b is slot b and its tail slot tail_slot + b, tail_slot = n_barcodes rounded up to 32."""
    if 2 * n_barcodes <= 32:
        chunks = 64 // (2 * n_barcodes)
        return chunks, 1, n_barcodes * chunks, -(-window // chunks)
    tail_slot = -(-n_barcodes // 32) * 32
    return 1, -(-(tail_slot + n_barcodes) // 64), tail_slot, window
# talc_umi_row (docs/umi.md)
UMI_DTYPE = np.dtype([("end", "u1"), ("err", "u1"), ("other_err", "u1"), ("umi_len", "u1"), ("start", "<u4"), ("stop", "<u4"),
                      ("kept_start", "<u4"), ("kept_len", "<u4"), ("umi", "S32"), ("pad_", "<u4")])
UMI_NONE, UMI_HEAD, UMI_TAIL = range(3)
UMI_DEFAULT_WINDOW = 256
# the default of the command line and of Context.set_umi (docs/umi.md, "The default max_error_pct"; tools/umi_defaults.py)
UMI_DEFAULT_ERR = 10
# talc_support_params (docs/base_support.md)
SUPPORT_RAW, SUPPORT_RECORD = 0, 1
# the k-mer spectrum (docs/kmer_spectrum.md): high 0 means the default; the largest high the kernel's LDS histogram holds
SPECTRUM_DEFAULT_HIGH, SPECTRUM_MAX_HIGH = 10000, 16382
EDIT_LETTERS = {EDIT_I: "I", EDIT_D: "D", EDIT_EQ: "=", EDIT_X: "X"}


def cigar_text(ops):
    """The ops of one read as text, e.g. 812=1X40=2D; '*' for none."""
    return "".join("%d%s" % (int(o) >> 4, EDIT_LETTERS[int(o) & 15]) for o in ops) or "*"


class TalcError(RuntimeError):
    """`code`: the library's talc_error (negative), or None where the wrapper itself refuses."""

    def __init__(self, message, code=None):
        super().__init__(message)
        self.code = code


class SupportParams(C.Structure):
    _fields_ = [("source", C.c_uint32), ("phred", C.c_uint32), ("qmin", C.c_uint32), ("qmax", C.c_uint32)]


class SpectrumStats(C.Structure):
    """talc_spectrum_stats (docs/kmer_spectrum.md)"""
    _fields_ = [("distinct", C.c_uint64), ("unique", C.c_uint64), ("total", C.c_uint64), ("max_count", C.c_uint64)]

    def as_tuple(self):
        return (int(self.distinct), int(self.unique), int(self.total), int(self.max_count))


class Params(C.Structure):
    _fields_ = [
        ("k", C.c_uint32),
        ("min_count", C.c_uint32),
        ("alpha", C.c_double),
        ("window_size", C.c_uint32),
        ("sr_error_rate", C.c_double),
        ("min_inner_score", C.c_double),
        ("min_border_score", C.c_double),
        ("max_nb_competing_paths", C.c_uint32),
        ("use_junctions", C.c_int32),
        ("reverse", C.c_int32),
        ("min_start_anchors", C.c_uint32),
        ("max_start_anchors", C.c_uint32),
        ("max_in_count", C.c_uint32),
        ("max_nb_border_paths", C.c_uint32),
        ("max_nb_inner_paths", C.c_uint32),
        ("check_interval", C.c_uint32),
        ("allowed_failure_rate", C.c_double),
        ("max_nb_border_failures", C.c_int32),
        ("coloured_count_thr", C.c_uint32),
        ("max_border_length", C.c_uint32),
    ]


class Timing(C.Structure):
    _fields_ = [
        ("encode_ms", C.c_float),
        ("coverage_ms", C.c_float),
        ("structure_ms", C.c_float),
        ("search_ms", C.c_float),
        ("emit_ms", C.c_float),
        ("retry_ms", C.c_float),
        ("n_kmers", C.c_uint64),
        ("n_bases", C.c_uint64),
        ("n_trail_steps", C.c_uint64),
        ("n_dp_cells", C.c_uint64),
        ("n_retried", C.c_uint32),
        ("n_failed", C.c_uint32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


def _abi():
    """Every symbol include/talc_hip.h declares: name -> (restype, argtypes).  Handles and buffers are void pointers."""
    vp, u64, u32, i32, txt = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_char_p
    par, out, stats = C.POINTER(Params), C.POINTER(C.c_void_p), C.POINTER(SpectrumStats)
    return {
        "talc_abi_version": (i32, []),
        "talc_last_error": (txt, []),
        "talc_params_default": (i32, [par]),
        "talc_device_count": (i32, []),
        "talc_pinned_alloc": (vp, [u64]),
        "talc_pinned_free": (None, [vp]),
        "talc_table_build": (i32, [txt, txt, par, out, vp]),
        "talc_table_from_arrays": (i32, [vp, vp, u64, par, out]),
        "talc_table_build_device": (i32, [txt, txt, par, i32, out, vp]),
        "talc_table_from_arrays_device": (i32, [vp, vp, u64, par, i32, out]),
        "talc_table_colour": (i32, [vp, vp, vp, u64]),
        "talc_table_decolour_repeats": (i32, [vp]),
        "talc_table_size": (u64, [vp]),
        "talc_table_device_bytes": (u64, [vp]),
        "talc_table_upload": (i32, [vp, i32]),
        "talc_table_capacity": (u64, [vp]),
        "talc_table_image_bytes": (u64, [vp]),
        "talc_table_export_device": (i32, [vp, i32, vp, vp]),
        "talc_table_import_device": (i32, [par, u64, u64, vp, vp, i32, out]),
        "talc_table_lookup_batch": (i32, [vp, i32, vp, u64, vp, vp]),
        "talc_table_next_counts_batch": (i32, [vp, i32, vp, u64, i32, vp, vp]),
        "talc_table_lookup_host_batch": (i32, [vp, vp, u64, vp, vp]),
        "talc_table_fetch_walk": (i32, [vp, i32, i32, vp, u64]),
        "talc_table_destroy": (None, [vp]),
        "talc_ctx_create": (i32, [vp, par, i32, out]),
        "talc_ctx_destroy": (None, [vp]),
        "talc_batch_create": (i32, [vp, vp, vp, u32, out]),
        "talc_batch_destroy": (None, [vp]),
        "talc_batch_coverage": (i32, [vp, vp]),
        "talc_batch_fetch_coverage": (i32, [vp, vp, vp, vp, vp, vp]),
        "talc_batch_fetch_coverage_degrees": (i32, [vp, vp, vp]),
        "talc_batch_structure": (i32, [vp, vp]),
        "talc_batch_fetch_structure": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp]),
        "talc_batch_order": (i32, [vp, vp, vp, vp]),
        "talc_batch_num_kmers": (u64, [vp]),
        "talc_batch_num_bases": (u64, [vp]),
        "talc_batch_correct": (i32, [vp, vp]),
        "talc_batch_corrected_bytes": (u64, [vp]),
        "talc_batch_fetch_corrected": (i32, [vp, vp, vp, u64, vp, vp]),
        "talc_batch_copy_corrected_device": (i32, [vp, vp, vp, u64, vp, vp]),
        "talc_batch_fetch_read_stats": (i32, [vp, vp, vp]),
        "talc_correct_batch": (i32, [vp, vp, vp, u32, vp, u64, vp, vp]),
        "talc_ctx_get_timing": (i32, [vp, C.POINTER(Timing)]),
        "talc_batch_trace_read": (C.c_int64, [vp, vp, u32, vp, u64]),
        "talc_test_dp": (i32, [vp, i32, txt, i32, txt, i32, i32, i32, i32, i32, vp]),
        "talc_counter_create": (i32, [par, i32, u64, out]),
        "talc_counter_add": (i32, [vp, vp, vp, u32]),
        "talc_counter_stats": (i32, [vp, vp]),
        "talc_counter_fetch": (i32, [vp, u32, vp, vp, u64, vp]),
        "talc_counter_build_table": (i32, [vp, txt, out, vp]),
        "talc_counter_destroy": (None, [vp]),
        "talc_counter_set_both_strands": (i32, [vp, i32]),
        "talc_counter_add_counts": (i32, [vp, vp, vp, u64]),
        "talc_table_build_device_both_strands": (i32, [txt, txt, par, i32, out, vp]),
        "talc_table_from_arrays_device_both_strands": (i32, [vp, vp, u64, par, i32, out]),
        "talc_counter_set_filter": (i32, [vp, u32, txt, u32, u32]),
        "talc_counter_add_fastq": (i32, [vp, vp, vp, vp, u32]),
        "talc_counter_filter_stats": (i32, [vp, vp]),
        "talc_test_counter_mask": (i32, [vp, vp, vp, vp, u32, vp, vp]),
        "talc_ctx_set_map": (i32, [vp, i32]),
        "talc_batch_num_segments": (u64, [vp]),
        "talc_batch_fetch_map": (i32, [vp, vp, vp, u64, vp]),
        "talc_batch_fetch_corrected_masked": (i32, [vp, vp, vp, u64, vp, vp]),
        "talc_ctx_get_map_timing": (i32, [vp, vp, vp]),
        "talc_batch_solidity": (i32, [vp, vp]),
        "talc_batch_fetch_solidity": (i32, [vp, vp, vp, vp]),
        "talc_ctx_get_solidity_timing": (i32, [vp, vp, vp]),
        "talc_batch_pieces": (i32, [vp, vp, i32, u32, i32]),
        "talc_batch_num_pieces": (u64, [vp]),
        "talc_batch_pieces_bytes": (u64, [vp]),
        "talc_batch_fetch_pieces": (i32, [vp, vp, vp, u64, vp, vp, u64, vp]),
        "talc_ctx_get_pieces_timing": (i32, [vp, vp, vp]),
        "talc_batch_edits": (i32, [vp, vp, u64]),
        "talc_batch_num_edit_ops": (u64, [vp]),
        "talc_batch_fetch_edits": (i32, [vp, vp, vp, u64, vp, vp]),
        "talc_ctx_get_edits_timing": (i32, [vp, vp, vp]),
        "talc_test_batch_edits": (i32, [vp, vp, u64, u64]),
        "talc_test_edit_script": (i32, [vp, txt, u32, txt, u32, u64, vp, u64, vp, vp]),
        "talc_test_parse_text": (i32, [txt, u32, u32, i32, i32, u64, i32, vp, vp, u64, vp, vp, vp]),
        "talc_ctx_set_auto_strand": (i32, [vp, i32]),
        "talc_batch_strand": (i32, [vp, vp]),
        "talc_batch_fetch_strand": (i32, [vp, vp, vp]),
        "talc_ctx_get_strand_timing": (i32, [vp, vp]),
        "talc_batch_support": (i32, [vp, vp, C.POINTER(SupportParams)]),
        "talc_batch_support_bytes": (u64, [vp]),
        "talc_batch_fetch_support": (i32, [vp, vp, vp, u64, vp]),
        "talc_ctx_get_support_timing": (i32, [vp, vp]),
        "talc_ctx_set_ends": (i32, [vp, txt, u32, u32, u32]),
        "talc_batch_ends": (i32, [vp, vp]),
        "talc_batch_fetch_ends": (i32, [vp, vp, vp]),
        "talc_batch_create_clipped": (i32, [vp, vp, vp, u32, out]),
        "talc_ctx_get_ends_timing": (i32, [vp, vp, vp]),
        "talc_ctx_set_chimera": (i32, [vp, i32, u32, u32]),
        "talc_batch_chimera": (i32, [vp, vp]),
        "talc_batch_num_chimera_hits": (u64, [vp]),
        "talc_batch_fetch_chimera": (i32, [vp, vp, vp, u64, vp]),
        "talc_batch_create_split": (i32, [vp, vp, vp, u32, i32, out]),
        "talc_batch_num_split_pieces": (u64, [vp]),
        "talc_batch_fetch_split": (i32, [vp, vp, vp, vp]),
        "talc_ctx_get_chimera_timing": (i32, [vp, vp, vp]),
        "talc_ctx_set_demux": (i32, [vp, txt, u32, u32, u32, i32]),
        "talc_batch_demux": (i32, [vp, vp]),
        "talc_batch_fetch_demux": (i32, [vp, vp, vp]),
        "talc_ctx_get_demux_timing": (i32, [vp, vp]),
        "talc_ctx_set_umi": (i32, [vp, txt, u32, u32]),
        "talc_batch_umi": (i32, [vp, vp]),
        "talc_batch_fetch_umi": (i32, [vp, vp, vp]),
        "talc_ctx_get_umi_timing": (i32, [vp, vp]),
        "talc_test_set_poison": (i32, [i32, u32]),
        "talc_test_get_poison": (i32, [vp, vp]),
        "talc_test_guard_report": (i32, [vp]),
        "talc_test_cache_reuses": (u64, []),
        "talc_test_guard_selftest": (i32, [vp]),
        "talc_test_fail_alloc": (i32, [u32, C.c_int64, u32, i32]),
        "talc_test_alloc_report": (i32, [vp]),
        "talc_test_retry_report": (i32, [vp, vp]),
        "talc_counter_histo": (i32, [vp, u32, vp, stats]),
        "talc_counter_get_histo_timing": (i32, [vp, vp]),
        "talc_table_histo": (i32, [vp, i32, u32, vp, stats]),
        "talc_spectrum_threshold": (i32, [vp, u32, u32, u32, vp, vp]),
        "talc_counter_set_min_count": (i32, [vp, u32]),
    }


ABI = _abi()
ABI_SYMBOLS = list(ABI)


def lib_path():
    # TALC_LIB selects another build of the same library (e.g. the -DTALC_PROF diagnostic build)
    return os.environ.get("TALC_LIB") or os.path.join(_build.OUT, "libtalc_hip.so")


def lib():
    """Load libtalc_hip.so (built in-tree by talc_amd.build); raises if it is missing."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise TalcError("libtalc_hip.so is missing: run `python -m talc_amd.build` (needs hipcc); "
                            "there is no CPU fallback for the correction path")
        L = C.CDLL(path)
        # (a TALC_LIB build of a parent commit that lacks a symbol still loads, for an A/B; asking it for that call raises)
        for name, (restype, argtypes) in ABI.items():
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = restype, argtypes
        _LIB = L
    return _LIB


ERR_NOMEM = -3          # TALC_ERR_NOMEM (docs/out_of_memory.md)
WARN_READ_ERRORS = 1   # TALC_WARN_READ_ERRORS: the batch is valid, some reads carry READ_ERROR


def _chk(rc):
    """Negative codes are errors; positive ones (TALC_WARN_READ_ERRORS) are returned to the caller."""
    if rc < 0:
        raise TalcError("libtalc_hip error %d: %s" % (rc, lib().talc_last_error().decode(errors="replace")), rc)
    return rc


def default_params(**kw):
    p = Params()
    _chk(lib().talc_params_default(C.byref(p)))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError("unknown parameter " + k)
        setattr(p, k, v)
    return p


def device_count():
    return int(lib().talc_device_count())


def poison_setting():
    """Test hook: (byte, guard bytes) of the poison setting as it is now; byte is -1 when it is off."""
    b, g = C.c_int(), C.c_uint32()
    _chk(lib().talc_test_get_poison(C.byref(b), C.byref(g)))
    return b.value, g.value


@contextlib.contextmanager
def poisoned(byte, guard=256):
    """Test hook: inside the block every device buffer the library hands out is filled with `byte` (0 .. 255) and sits between
    red zones of `guard` bytes (a multiple of 256) that are checked when it is given back (guard_report()).  Process-wide;
    always switched off again."""
    _chk(lib().talc_test_set_poison(int(byte), int(guard)))
    try:
        yield
    finally:
        _chk(lib().talc_test_set_poison(-1, 0))


def guard_report():
    """Test hook: what the red-zone checks have seen since the library was loaded: dict of checked, violations, first_bytes,
    first_side (0 in front of the buffer, 1 behind it), first_offset, and reused (requests a context's cache served with a
    buffer used before, while the setting was on)."""
    r = np.zeros(4, dtype=np.uint64)
    _chk(lib().talc_test_guard_report(r.ctypes.data))
    return dict(checked=int(r[0]), violations=int(r[1]), first_bytes=int(r[2]), first_side=int(r[3]) >> 32,
                first_offset=int(r[3]) & 0xFFFFFFFF, reused=int(lib().talc_test_cache_reuses()))


def guard_selftest():
    """Test hook (needs a GPU, inside poisoned()): dict of fills (15: every byte read back as specified), violations (2) and
    the (side, offset) of the two it caused: behind the first buffer, in front of the second."""
    r = np.zeros(4, dtype=np.uint64)
    _chk(lib().talc_test_guard_selftest(r.ctypes.data))
    where = [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in r[2:]]
    return dict(fills=int(r[0]), violations=int(r[1]), behind=where[0], in_front=where[1])


KIND_DEVICE, KIND_PINNED = 1, 2                                          # talc_test_fail_alloc's kinds
OWNER_DEVBUF, OWNER_DEVCACHE, OWNER_PINNED, OWNER_HOST_BLOCK = 1, 2, 3, 4   # talc_test_alloc_report's owners


@contextlib.contextmanager
def failing_allocs(kinds, skip, count, real=False):
    """Test hook (docs/out_of_memory.md): inside the block the library's allocation requests of `kinds` (1 device, 2 pinned
    host, 3 both) are numbered from 0 and requests skip .. skip + count - 1 fail (count 0: they are only counted,
    alloc_report()); real: the runtime is asked for 2^60 bytes, so that its own error state is that of a true failure.
    Process-wide; always switched off again; the report keeps what the block saw until the hook is armed again."""
    _chk(lib().talc_test_fail_alloc(int(kinds), int(skip), int(count), 1 if real else 0))
    try:
        yield
    finally:
        _chk(lib().talc_test_fail_alloc(0, 0, 0, 0))


def alloc_report():
    """Test hook: dict of device (requests seen since the hook was last armed), pinned, injected, owner and bytes of the last
    injected failure, runtime_code of the last real failure, live (device buffers the library holds now) and kinds (0: off).
    Switching the hook off keeps the numbers: after a failing_allocs block they are what the block saw.  Needs no GPU."""
    r = np.zeros(8, dtype=np.uint64)
    _chk(lib().talc_test_alloc_report(r.ctypes.data))
    return dict(device=int(r[0]), pinned=int(r[1]), injected=int(r[2]), owner=int(r[3]), bytes=int(r[4]), runtime_code=int(r[5]),
                live=int(r[6].astype(np.int64)), kinds=int(r[7]))


def parse_text_hook(path, k, min_count=2, where=1, device=0, chunk_bytes=32 << 20, reader_threads=8, arrays=True):
    """Test hook: the text-dump parser alone on a file of any size.  where=1: the file goes to GPU `device` in chunks of
    chunk_bytes read by at most reader_threads threads and is parsed there; where=0: the host parser, unfiltered (no GPU).
    Returns a dict: kmers u64[n] and counts u32[n] in file order (None with arrays=False), n_lines, kept, and flags (device:
    != 0 when a line is not canonical) or nread / nbad (host)."""
    L = lib()
    n, kept, flags = C.c_uint64(), C.c_uint64(), C.c_uint64()
    args = (path.encode(), int(k), int(min_count), int(where), int(device), int(chunk_bytes), int(reader_threads))
    _chk(L.talc_test_parse_text(*args, None, None, 0, C.byref(n), C.byref(kept), C.byref(flags)))
    out = {"kmers": None, "counts": None}
    if arrays:
        km, ct = np.zeros(max(n.value, 1), dtype=np.uint64), np.zeros(max(n.value, 1), dtype=np.uint32)
        _chk(L.talc_test_parse_text(*args, km.ctypes.data, ct.ctypes.data, n.value, C.byref(n), C.byref(kept), C.byref(flags)))
        out = {"kmers": km[:n.value], "counts": ct[:n.value]}
    out.update(n_lines=n.value, kept=kept.value)
    if where:
        out["flags"] = flags.value
    else:
        out.update(nread=n.value + (flags.value >> 32), nbad=flags.value & 0xFFFFFFFF)
    return out


class PinnedArray:
    """A uint8 numpy view over page-locked host memory of the library (talc_pinned_alloc)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self._p = lib().talc_pinned_alloc(max(self.nbytes, 1))
        if not self._p:
            raise TalcError("talc_pinned_alloc(%d) failed: %s" % (nbytes, lib().talc_last_error().decode(errors="replace")), ERR_NOMEM)
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(self.nbytes, 1)).from_address(self._p))[: self.nbytes]

    def close(self):
        if self._p:
            self.array = None
            lib().talc_pinned_free(C.c_void_p(self._p))
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Owner:
    """What owns one object of the library: `_h` is its handle, `_destroy` the name of the call that gives it back."""
    _h = None

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _histo(call, *args):
    """One spectrum call (its own arguments end with `high`): (hist u64[high + 2], (distinct, unique, total, max_count))."""
    hist = np.zeros(min(args[-1] or SPECTRUM_DEFAULT_HIGH, SPECTRUM_MAX_HIGH) + 2, dtype=np.uint64)   # (a high out of range is refused)
    st = SpectrumStats()
    _chk(call(*args, hist.ctypes.data, C.byref(st)))
    return hist, st.as_tuple()


class Table(_Owner):
    """The SR k-mer table (replaces buildCDBG, Jellyfish.cpp:236-295)."""
    _destroy = "talc_table_destroy"

    def __init__(self, handle, params):
        self._h = handle
        self.params = params

    @classmethod
    def from_arrays(cls, kmers, counts, params, device=None, both_strands=False):
        """device=None: host builder; device=d: insertion on GPU d (same content).  both_strands (docs/both_strands.md,
        device only): the counts are summed over every k-mer and its reverse complement on the GPU, the filter applies
        to the sum and both are stored."""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        h = C.c_void_p()
        if both_strands:
            if device is None:
                raise TalcError("a table on both strands is folded on the GPU: give a device (there is no host fold)")
            _chk(lib().talc_table_from_arrays_device_both_strands(kmers.ctypes.data, counts.ctypes.data, len(kmers), C.byref(params),
                                                                  int(device), C.byref(h)))
        elif device is None:
            _chk(lib().talc_table_from_arrays(kmers.ctypes.data, counts.ctypes.data, len(kmers), C.byref(params), C.byref(h)))
        else:
            _chk(lib().talc_table_from_arrays_device(kmers.ctypes.data, counts.ctypes.data, len(kmers), C.byref(params),
                                                     int(device), C.byref(h)))
        return cls(h, params)

    @classmethod
    def from_files(cls, dump, junctions, params, device=None, both_strands=False):
        """both_strands (device only): the dump's counts folded over reverse complements on the GPU, as from_arrays."""
        h = C.c_void_p()
        st = np.zeros(3, dtype=np.int64)
        if both_strands:
            if device is None:
                raise TalcError("a table on both strands is folded on the GPU: give a device (there is no host fold)")
            _chk(lib().talc_table_build_device_both_strands(dump.encode(), junctions.encode() if junctions else None, C.byref(params),
                                                            int(device), C.byref(h), st.ctypes.data))
        elif device is None:
            _chk(lib().talc_table_build(dump.encode(), junctions.encode() if junctions else None, C.byref(params), C.byref(h), st.ctypes.data))
        else:
            _chk(lib().talc_table_build_device(dump.encode(), junctions.encode() if junctions else None, C.byref(params),
                                               int(device), C.byref(h), st.ctypes.data))
        t = cls(h, params)
        t.build_stats = st
        return t

    def colour(self, jkmers, jcounts):
        jkmers = np.ascontiguousarray(jkmers, dtype=np.uint64)
        jcounts = np.ascontiguousarray(jcounts, dtype=np.int64)
        _chk(lib().talc_table_colour(self._h, jkmers.ctypes.data, jcounts.ctypes.data, len(jkmers)))

    def decolour_repeats(self):
        _chk(lib().talc_table_decolour_repeats(self._h))

    def __len__(self):
        return int(lib().talc_table_size(self._h))

    @property
    def device_bytes(self):
        return int(lib().talc_table_device_bytes(self._h))

    def upload(self, device=0):
        _chk(lib().talc_table_upload(self._h, device))

    @property
    def capacity(self):
        return int(lib().talc_table_capacity(self._h))

    @property
    def image_bytes(self):
        """Bytes of each of the two bucket tables (RIGHT, LEFT) of the device image."""
        return int(lib().talc_table_image_bytes(self._h))

    def export_device(self, device, ptr_right, ptr_left):
        """Copy the image on `device` into two caller-owned device buffers of image_bytes each."""
        _chk(lib().talc_table_export_device(self._h, int(device), C.c_void_p(ptr_right), C.c_void_p(ptr_left)))

    @classmethod
    def import_device(cls, params, capacity, n_kmers, ptr_right, ptr_left, device):
        """A table on `device` from an exported image (two device buffers; they are copied)."""
        h = C.c_void_p()
        _chk(lib().talc_table_import_device(C.byref(params), int(capacity), int(n_kmers), C.c_void_p(ptr_right),
                                            C.c_void_p(ptr_left), int(device), C.byref(h)))
        return cls(h, params)

    def lookup(self, kmers, device=0):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        c = np.empty(len(kmers), dtype=np.uint32)
        j = np.empty(len(kmers), dtype=np.uint32)
        _chk(lib().talc_table_lookup_batch(self._h, device, kmers.ctypes.data, len(kmers), c.ctypes.data, j.ctypes.data))
        return c, j

    def lookup_host(self, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        c = np.empty(len(kmers), dtype=np.uint32)
        j = np.empty(len(kmers), dtype=np.uint32)
        _chk(lib().talc_table_lookup_host_batch(self._h, kmers.ctypes.data, len(kmers), c.ctypes.data, j.ctypes.data))
        return c, j

    def next_counts(self, kmers, direction, device=0):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        c = np.empty((len(kmers), 4), dtype=np.uint32)
        j = np.empty((len(kmers), 4), dtype=np.uint32)
        _chk(lib().talc_table_next_counts_batch(self._h, device, kmers.ctypes.data, len(kmers), int(direction), c.ctypes.data, j.ctypes.data))
        return c, j

    WALK_DTYPE = np.dtype([("key", "<u8"), ("lvl", "<u2", (12,))])

    def fetch_walk(self, direction, device=0):
        """Test hook: the walk table of one direction (0 LEFT, 1 RIGHT) of the copy on `device`, one WALK_DTYPE record
        per bucket; TalcError when that copy has no walk tables."""
        w = np.empty(self.capacity, dtype=self.WALK_DTYPE)
        _chk(lib().talc_table_fetch_walk(self._h, int(device), int(direction), w.ctypes.data, w.nbytes))
        return w

    def histo(self, device=0, high=0):
        """The count spectrum of the k-mers the table stores, from its image on `device` (staged or uploaded; TalcError
        without one): (hist u64[high + 2], (distinct, unique, total, max_count)) as KmerCounter.histo."""
        return _histo(lib().talc_table_histo, self._h, int(device), int(high))


class KmerCounter(_Owner):
    """Short-read k-mer counter on GPU `device` (replaces `jellyfish count -m K` + `dump -c`; docs/kmer_counting.md):
    every window of K bases of ACGTacgt inside one record counts once, directional, 2 bits per base.  both_strands
    (docs/both_strands.md): every observation counts for the canonical k-mer min(x, rc(x)); fetch returns canonical k-mers
    and build_table stores each kept one with its reverse complement."""
    _destroy = "talc_counter_destroy"

    def __init__(self, params, device=0, expected_distinct=0, both_strands=False):
        self.params = params
        self.device = int(device)
        self.both_strands = bool(both_strands)
        h = C.c_void_p()
        _chk(lib().talc_counter_create(C.byref(params), self.device, int(expected_distinct), C.byref(h)))
        self._h = h
        if self.both_strands:
            self.set_both_strands(True)

    def set_both_strands(self, on=True):
        """Before the first add / add_counts only (TalcError afterwards)."""
        _chk(lib().talc_counter_set_both_strands(self._h, 1 if on else 0))
        self.both_strands = bool(on)

    def add_counts(self, kmers, counts):
        """Counted k-mers (packed u64, u32): counts[i] is added to kmers[i], or to its canonical form on a both-strands counter."""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        if len(kmers) != len(counts):
            raise ValueError("kmers and counts differ in length")
        _chk(lib().talc_counter_add_counts(self._h, kmers.ctypes.data, counts.ctypes.data, len(kmers)))

    def set_filter(self, min_qual=0, adapters=(), min_overlap=0, max_error_pct=10):
        """The short-read filter (docs/sr_filter.md), before the first add only: bases with a Phred+33 quality below min_qual
        and everything from the first match of one of `adapters` (str / bytes, or a sequence of up to 4) are counted as N.
        min_overlap 0 is the default 5.  No adapters and min_qual 0 switch it off."""
        if isinstance(adapters, (str, bytes)):
            adapters = [adapters]
        text = b",".join(a.encode() if isinstance(a, str) else bytes(a) for a in adapters)
        if len(adapters) and not text:
            text = b","      # (an empty adapter is refused by the library, not dropped here)
        _chk(lib().talc_counter_set_filter(self._h, int(min_qual), text, int(min_overlap), int(max_error_pct)))

    @staticmethod
    def _batch(bases, offsets, quals):
        if isinstance(bases, (bytes, bytearray)):
            bases = np.frombuffer(bases, dtype=np.uint8)
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if quals is not None:
            if isinstance(quals, (bytes, bytearray)):
                quals = np.frombuffer(quals, dtype=np.uint8)
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
            if len(quals) != len(bases):
                raise ValueError("one quality per base is expected")
        return bases, offsets, quals

    def add(self, bases, offsets, quals=None):
        """Queue a batch of records (bases: uint8 / bytes concatenated, offsets: u64[n+1]; quals: one Phred+33 byte per base,
        for the filter's quality floor); the arrays may be reused at once."""
        bases, offsets, quals = self._batch(bases, offsets, quals)
        if quals is None:
            _chk(lib().talc_counter_add(self._h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1))
        else:
            _chk(lib().talc_counter_add_fastq(self._h, bases.ctypes.data, quals.ctypes.data, offsets.ctypes.data, len(offsets) - 1))

    def filter_stats(self):
        """(records filtered, records clipped, bytes clipped, bytes below the quality floor ahead of the clip)."""
        st = np.zeros(4, dtype=np.uint64)
        _chk(lib().talc_counter_filter_stats(self._h, st.ctypes.data))
        return tuple(int(x) for x in st)

    def mask(self, bases, offsets, quals=None):
        """Test hook: the filter alone on one batch: (masked bytes uint8, without separators; clip u32[n]).  Counts nothing."""
        bases, offsets, quals = self._batch(bases, offsets, quals)
        n = len(offsets) - 1
        masked = np.zeros(max(int(offsets[-1] - offsets[0]), 1), dtype=np.uint8)
        clip = np.zeros(max(n, 1), dtype=np.uint32)
        _chk(lib().talc_test_counter_mask(self._h, bases.ctypes.data, quals.ctypes.data if quals is not None else None,
                                          offsets.ctypes.data, n, masked.ctypes.data, clip.ctypes.data))
        return masked[: int(offsets[-1] - offsets[0])], clip[:n]

    def stats(self):
        """(windows counted, distinct k-mers, distinct k-mers with count >= params.min_count)."""
        st = np.zeros(3, dtype=np.uint64)
        _chk(lib().talc_counter_stats(self._h, st.ctypes.data))
        return tuple(int(x) for x in st)

    def fetch(self, min_count=1):
        """(kmers u64, counts u32) of the k-mers with count >= min_count, in no particular order."""
        n = C.c_uint64()
        _chk(lib().talc_counter_fetch(self._h, int(min_count), None, None, 0, C.byref(n)))
        kmers = np.empty(max(n.value, 1), dtype=np.uint64)
        counts = np.empty(max(n.value, 1), dtype=np.uint32)
        _chk(lib().talc_counter_fetch(self._h, int(min_count), kmers.ctypes.data, counts.ctypes.data, n.value, C.byref(n)))
        return kmers[: n.value], counts[: n.value]

    def histo(self, high=0):
        """The count spectrum (docs/kmer_spectrum.md; `jellyfish histo`): (hist u64[high + 2], (distinct, unique, total,
        max_count)).  hist[c] = the k-mers with count c, hist[high + 1] those above high; high 0 is 10000.  The counter is
        not spent and nothing it holds changes."""
        return _histo(lib().talc_counter_histo, self._h, int(high))

    def histo_timing(self):
        """Device time (ms) of the last k_count_histo of this counter."""
        ms = C.c_float()
        _chk(lib().talc_counter_get_histo_timing(self._h, C.byref(ms)))
        return ms.value

    def set_min_count(self, min_count):
        """Replaces params.min_count for stats()[2] and build_table(): the counter gets its own copy of the parameters, and
        build_table() hands that copy to the Table (a Context on it must be created with table.params)."""
        _chk(lib().talc_counter_set_min_count(self._h, int(min_count)))
        own = Params.from_buffer_copy(self.params)
        own.min_count = int(min_count)
        self.params = own

    def build_table(self, junctions=None):
        """The table of the k-mers with count >= params.min_count (staged on the counter's GPU); the counter is spent."""
        h = C.c_void_p()
        st = np.zeros(3, dtype=np.int64)
        _chk(lib().talc_counter_build_table(self._h, junctions.encode() if junctions else None, C.byref(h), st.ctypes.data))
        t = Table(h, self.params)
        t.build_stats = st
        return t


def spectrum_threshold(hist, limit=0, fallback=2):
    """(chosen, valley) of a spectrum as histo() returns it (hist[len - 1] is the catch-all bin): the first local minimum,
    valley = the smallest c in [1, min(limit, high - 1)] with hist[c + 1] > 0 and hist[c] <= hist[c + 1], 0 when there is
    none; chosen = max(2, valley), or fallback without a valley.  limit 0 is 32.  Host only, needs no GPU."""
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    chosen, valley = C.c_uint32(), C.c_uint32()
    _chk(lib().talc_spectrum_threshold(hist.ctypes.data, max(len(hist) - 2, 0), int(limit), int(fallback), C.byref(chosen), C.byref(valley)))
    return chosen.value, valley.value


def mask_batch(bases, offsets, quals=None, min_qual=0, adapters=(), min_overlap=0, max_error_pct=10, params=None, device=0):
    """Test hook (talc_test_counter_mask): the short-read filter alone on one batch, on a counter of its own.  Returns
    (masked bytes without separators, clip u32[n])."""
    c = KmerCounter(params or default_params(), device)
    try:
        c.set_filter(min_qual, adapters, min_overlap, max_error_pct)
        return c.mask(bases, offsets, quals)
    finally:
        c.close()


class Context(_Owner):
    _destroy = "talc_ctx_destroy"

    def __init__(self, table, params=None, device=0):
        self.table = table
        self.params = params or table.params
        self.device = device
        h = C.c_void_p()
        _chk(lib().talc_ctx_create(table._h, C.byref(self.params), device, C.byref(h)))
        self._h = h
        self._auto = False   # auto_strand()

    def timing(self):
        t = Timing()
        _chk(lib().talc_ctx_get_timing(self._h, C.byref(t)))
        return t

    def retry_report(self):
        """Test hook: the retry passes of the context's last correction: dict of x8 and x64 (reads each stage searched), left
        (reads still flagged behind the last stage that ran: timing().n_failed) and refused (stages that did not fit)."""
        r = np.zeros(4, dtype=np.uint32)
        _chk(lib().talc_test_retry_report(self._h, r.ctypes.data))
        return dict(x8=int(r[0]), x64=int(r[1]), left=int(r[2]), refused=int(r[3]))

    def record_map(self, on=True):
        """Later corrections of this context keep the correction map (Batch.fetch_map, fetch_corrected(soft_mask=True))."""
        _chk(lib().talc_ctx_set_map(self._h, 1 if on else 0))

    def map_timing(self):
        """(k_pack_map ms, k_mask_case ms) of the context's last map kernels."""
        a, b = C.c_float(), C.c_float()
        _chk(lib().talc_ctx_get_map_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def solidity_timing(self):
        """(raw ms, corrected ms): device time of the two k_solidity launches of the context's last Batch.solidity()."""
        a, b = C.c_float(), C.c_float()
        _chk(lib().talc_ctx_get_solidity_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def pieces_timing(self):
        """(k_piece_count ms, k_piece_pack ms) of the context's last Batch.pieces()."""
        a, b = C.c_float(), C.c_float()
        _chk(lib().talc_ctx_get_pieces_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def auto_strand(self, on=True):
        """Later calls of this context take every read in the orientation the short reads support (docs/auto_strand.md;
        Batch.strand() says which).  TalcError when the context's params have reverse set."""
        _chk(lib().talc_ctx_set_auto_strand(self._h, 1 if on else 0))
        self._auto = bool(on)

    def strand_timing(self):
        """Device time (ms) of the context's last k_strand_vote."""
        a = C.c_float()
        _chk(lib().talc_ctx_get_strand_timing(self._h, C.byref(a)))
        return a.value

    def set_ends(self, adapters=(), max_error_pct=20, poly_min=0, window=512):
        """The long-read end clean-up (docs/read_ends.md): up to 4 adapters of 12..64 letters, found within max_error_pct
        (0..30) per cent of their length in edits inside the first / last `window` (32..4096) bytes, and a poly-T head /
        poly-A tail of at least poly_min (0: off, else 8..window) bases behind them.  No adapters and poly_min 0: off."""
        if isinstance(adapters, (str, bytes)):
            adapters = [adapters]
        text = ",".join(a.decode() if isinstance(a, bytes) else a for a in adapters)
        _chk(lib().talc_ctx_set_ends(self._h, text.encode(), int(max_error_pct), int(poly_min), int(window)))

    def ends_timing(self):
        """(k_read_ends ms, k_gather ms) of the context's last end scan and last clipped batch."""
        a, b = C.c_float(), C.c_float()
        _chk(lib().talc_ctx_get_ends_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_chimera(self, on=True, max_error_pct=10, min_piece=0):
        """The chimera scan (docs/chimeras.md): the adapters of set_ends searched over the whole of every read on both
        strands within max_error_pct (0..30) per cent of their length in edits; split batches drop pieces shorter than
        min_piece."""
        _chk(lib().talc_ctx_set_chimera(self._h, 1 if on else 0, int(max_error_pct), int(min_piece)))

    def chimera_timing(self):
        """(k_read_chimera ms, k_gather ms) of the context's last chimera scan and last split batch."""
        a, b = C.c_float(), C.c_float()
        _chk(lib().talc_ctx_get_chimera_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_demux(self, barcodes=(), max_error_pct=DEMUX_DEFAULT_ERR, min_margin=DEMUX_DEFAULT_MARGIN, window=DEMUX_DEFAULT_WINDOW, both_ends=False):
        """Barcode demultiplexing (docs/demux.md): 1..96 barcodes of one length (12..64 letters), searched within
        max_error_pct (0..30) per cent of that length in edits inside the first `window` (32..4096) bytes of every read and,
        reverse-complemented, inside the last; an end calls its best barcode when the runner-up is at least min_margin edits
        worse; both_ends: only reads whose two ends call the same barcode get it.  No barcodes: off."""
        if isinstance(barcodes, (str, bytes)):
            barcodes = [barcodes]
        text = ",".join(a.decode() if isinstance(a, bytes) else a for a in barcodes)
        _chk(lib().talc_ctx_set_demux(self._h, text.encode(), int(max_error_pct), int(min_margin), int(window), 1 if both_ends else 0))

    def demux_timing(self):
        """Device time (ms) of the context's last k_read_demux; 0.0 after a Batch.demux() that found its rows made."""
        a = C.c_float()
        _chk(lib().talc_ctx_get_demux_timing(self._h, C.byref(a)))
        return a.value

    def set_umi(self, pattern="", max_error_pct=UMI_DEFAULT_ERR, window=UMI_DEFAULT_WINDOW):
        """The UMI read-out (docs/umi.md): one pattern of 12..64 IUPAC letters (ACGTRYSWKMBDHVN) with 1..32 degenerate ones,
        searched within max_error_pct (0..30) per cent of its length in edits inside the first `window` (32..4096) bytes of
        every read and, reverse-complemented, inside the last; the alignment gives the read's bases under the degenerate
        letters.  batch(clip=True) then cuts the pattern off too.  No pattern: off."""
        text = pattern.decode() if isinstance(pattern, bytes) else pattern
        _chk(lib().talc_ctx_set_umi(self._h, text.encode(), int(max_error_pct), int(window)))

    def umi_timing(self):
        """Device time (ms) of the context's last k_read_umi; 0.0 after a Batch.umi() that found its rows made."""
        a = C.c_float()
        _chk(lib().talc_ctx_get_umi_timing(self._h, C.byref(a)))
        return a.value

    def support_timing(self):
        """Device time (ms) of the k_base_support launch of the context's last Batch.support()."""
        a = C.c_float()
        _chk(lib().talc_ctx_get_support_timing(self._h, C.byref(a)))
        return a.value

    def edits_timing(self):
        """(align ms, pack ms) of the context's last Batch.edits(): both runs of k_edit_align, k_edit_count + k_edit_pack."""
        a, b = C.c_float(), C.c_float()
        _chk(lib().talc_ctx_get_edits_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def test_edit_script(self, a, b, max_cells=0):
        """Test hook: (ops uint32[], distance) of one pair of ASCII sequences as one CORRECTED segment; distance -1 when
        the pair is over max_cells and was not aligned."""
        a = a if isinstance(a, bytes) else a.encode()
        b = b if isinstance(b, bytes) else b.encode()
        n, d = C.c_uint64(), C.c_int32()
        L = lib()
        _chk(L.talc_test_edit_script(self._h, a, len(a), b, len(b), int(max_cells), None, 0, C.byref(n), C.byref(d)))
        ops = np.zeros(max(n.value, 1), dtype=np.uint32)
        _chk(L.talc_test_edit_script(self._h, a, len(a), b, len(b), int(max_cells), ops.ctypes.data, n.value, C.byref(n), C.byref(d)))
        return ops[:n.value], d.value

    def batch(self, bases, offsets, clip=False, split=False):
        """clip: the batch is made from the reads' kept intervals (set_ends and / or set_umi, whose intervals combine;
        Batch.ends() and Batch.umi() then have the rows of the reads as given).
        split: its reads are the kept pieces of the given reads (set_chimera; Batch.split_pieces() says which); with clip
        too, every piece is clipped."""
        return Batch(self, bases, offsets, clip=clip, split=split)

    def test_dp(self, mode, a, b, p0=0, p1=0, p2=0, p3=0):
        out = np.zeros(max(12, p2) if (mode == 3 and p1) else 12, dtype=np.int32)   # (mode 3's table form: one word per record)
        a = a if isinstance(a, bytes) else a.encode()
        b = b if isinstance(b, bytes) else b.encode()
        _chk(lib().talc_test_dp(self._h, mode, a, len(a), b, len(b), p0, p1, p2, p3, out.ctypes.data))
        return out

    def correct(self, bases, offsets, out=None):
        """One-shot: returns (out uint8 ASCII, out_offsets, status)."""
        b = self.batch(bases, offsets)
        try:
            b.correct()
            return b.fetch_corrected(out)
        finally:
            b.close()


class Batch(_Owner):
    """A batch of reads resident in HBM."""
    _destroy = "talc_batch_destroy"

    def __init__(self, ctx, bases, offsets, clip=False, split=False):
        self.ctx = ctx
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.n_reads = self.n_source_reads = len(offsets) - 1
        h = C.c_void_p()
        if split:
            _chk(lib().talc_batch_create_split(ctx._h, bases.ctypes.data, offsets.ctypes.data, self.n_reads, 1 if clip else 0, C.byref(h)))
            self.n_reads = int(lib().talc_batch_num_split_pieces(h))   # (one read per kept piece)
        else:
            create = lib().talc_batch_create_clipped if clip else lib().talc_batch_create
            _chk(create(ctx._h, bases.ctypes.data, offsets.ctypes.data, self.n_reads, C.byref(h)))
        self._h = h
        self._corrected = False   # the batch holds the records of a correction (solidity() then has corrected rows)
        self._enc_auto = None     # the auto-strand setting the batch's codes were made under

    def _needs_codes(self):
        """A batch whose codes were made under the other auto-strand setting is encoded again, as if it were new."""
        if self._enc_auto is not None and self._enc_auto != self.ctx._auto:
            self._corrected = False
        self._enc_auto = self.ctx._auto

    @property
    def n_kmers(self):
        return int(lib().talc_batch_num_kmers(self._h))

    @property
    def n_bases(self):
        return int(lib().talc_batch_num_bases(self._h))

    def coverage(self):
        self._needs_codes()
        _chk(lib().talc_batch_coverage(self.ctx._h, self._h))

    def fetch_coverage(self):
        n = self.n_kmers
        c = np.empty(n, dtype=np.uint32)
        j = np.empty(n, dtype=np.uint32)
        ko = np.empty(self.n_reads + 1, dtype=np.uint64)
        nin = np.empty(self.n_reads, dtype=np.int32)
        _chk(lib().talc_batch_fetch_coverage(self.ctx._h, self._h, c.ctypes.data, j.ctypes.data, ko.ctypes.data, nin.ctypes.data))
        return c, j, ko, nin

    def fetch_coverage_degrees(self):
        """Test hook: uint8 per k-mer position (layout of fetch_coverage): right degree | left degree << 3 | known << 6."""
        d = np.zeros(max(self.n_kmers, 1), dtype=np.uint8)
        _chk(lib().talc_batch_fetch_coverage_degrees(self.ctx._h, self._h, d.ctypes.data))
        return d[: self.n_kmers]

    def structure(self):
        """Test hook: encode, coverage and the structure kernel; nothing of the search."""
        self._needs_codes()
        self._corrected = False
        _chk(lib().talc_batch_structure(self.ctx._h, self._h))

    def order(self):
        """Test hook, after structure(): (order u32[n], bucket u32[n], gap scale) — the work queue, every read's bucket
        and the batch's gap scale (in 1/256) as the device derived it."""
        n = self.n_reads
        order, bucket = np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint32)
        _chk(lib().talc_batch_order(self.ctx._h, self._h, order.ctypes.data, bucket.ctypes.data))
        return order[:n], bucket[:n], int(bucket[n])

    def fetch_structure(self):
        """Test hook, after structure(): dict of status i32[n], n_regions u32[n], lambda f64[n], in_span u32[n],
        region_offsets u64[n+1], regions u32[R, 2] (start, end), region_hits u32[R], head_counts u32[n, 16]."""
        n = self.n_reads
        out = dict(status=np.zeros(n, np.int32), n_regions=np.zeros(n, np.uint32), lam=np.zeros(n, np.float64),
                   in_span=np.zeros(n, np.uint32), region_offsets=np.zeros(n + 1, np.uint64),
                   head_counts=np.zeros((n, 16), np.uint32))
        L, h = lib(), self._h
        _chk(L.talc_batch_fetch_structure(self.ctx._h, h, out["status"].ctypes.data, out["n_regions"].ctypes.data, out["lam"].ctypes.data,
                                          out["in_span"].ctypes.data, out["region_offsets"].ctypes.data, None, None, 0,
                                          out["head_counts"].ctypes.data))
        R = int(out["region_offsets"][n])
        out["regions"] = np.zeros((R, 2), np.uint32)
        out["region_hits"] = np.zeros(R, np.uint32)
        if R:
            _chk(L.talc_batch_fetch_structure(self.ctx._h, h, None, None, None, None, None, out["regions"].ctypes.data,
                                              out["region_hits"].ctypes.data, R, None))
        return out

    def correct(self):
        """0, or WARN_READ_ERRORS when some reads exhausted the device scratch (status READ_ERROR, passed through)."""
        self._needs_codes()
        self._corrected = False
        rc = _chk(lib().talc_batch_correct(self.ctx._h, self._h))
        self._corrected = True
        return rc

    def fetch_corrected(self, out=None, soft_mask=False):
        """(records uint8 ASCII, offsets, status); `out`: a caller's uint8 buffer to fill (e.g. PinnedArray.array).
        soft_mask: the bases of RAW segments in lower case (needs Context.record_map() before the correction)."""
        total = int(lib().talc_batch_corrected_bytes(self._h))
        if out is None or len(out) < total:
            out = np.empty(max(total, 1), dtype=np.uint8)
        oo = np.empty(self.n_reads + 1, dtype=np.uint64)
        st = np.empty(self.n_reads, dtype=np.int32)
        fetch = lib().talc_batch_fetch_corrected_masked if soft_mask else lib().talc_batch_fetch_corrected
        _chk(fetch(self.ctx._h, self._h, out.ctypes.data, total, oo.ctypes.data, st.ctypes.data))
        return out[:total], oo, st

    @property
    def n_segments(self):
        return int(lib().talc_batch_num_segments(self._h))

    def fetch_map(self):
        """(segments as a SEGMENT_DTYPE array, offsets u64[n_reads + 1]): the correction map of the last correction."""
        so = np.empty(self.n_reads + 1, dtype=np.uint64)
        _chk(lib().talc_batch_fetch_map(self.ctx._h, self._h, None, 0, so.ctypes.data))
        n = int(so[self.n_reads])
        segs = np.empty(max(n, 1), dtype=SEGMENT_DTYPE)
        _chk(lib().talc_batch_fetch_map(self.ctx._h, self._h, segs.ctypes.data, n, so.ctypes.data))
        return segs[:n], so

    def solidity(self):
        """The solidity report (docs/solidity.md): (raw, corrected) as SOLIDITY_DTYPE arrays of one row per read — how
        much of the read, and of its record, the short reads support.  corrected is None on a batch that has not been
        corrected."""
        self._needs_codes()
        _chk(lib().talc_batch_solidity(self.ctx._h, self._h))
        raw = np.zeros(self.n_reads, dtype=SOLIDITY_DTYPE)
        cor = np.zeros(self.n_reads, dtype=SOLIDITY_DTYPE) if self._corrected else None
        _chk(lib().talc_batch_fetch_solidity(self.ctx._h, self._h, raw.ctypes.data, cor.ctypes.data if self._corrected else None))
        return raw, cor

    def support(self, source="record", phred=None):
        """Per-base support (docs/base_support.md): (bytes uint8, offsets u64[n_reads + 1]), one byte per base — of the
        records of the last correction (source="record", laid out as fetch_corrected's) or of the reads as they were
        given (source="raw").  The byte is cover, the number of solid k-mers that hold the base (0 .. K); with
        phred=(qmin, qmax) it is the quality character 33 + qmin + (qmax - qmin) * cover // span."""
        if source not in ("raw", "record"):
            raise ValueError("source must be 'raw' or 'record'")
        self._needs_codes()
        p = SupportParams(SUPPORT_RECORD if source == "record" else SUPPORT_RAW, 0, 0, 0)
        if phred is not None:
            lo, hi = phred
            if lo < 0 or hi < 0:
                raise ValueError("qualities are not negative")
            p.phred, p.qmin, p.qmax = 1, int(lo), int(hi)
        L = lib()
        _chk(L.talc_batch_support(self.ctx._h, self._h, C.byref(p)))
        total = int(L.talc_batch_support_bytes(self._h))
        out = np.empty(max(total, 1), dtype=np.uint8)
        oo = np.empty(self.n_reads + 1, dtype=np.uint64)
        _chk(L.talc_batch_fetch_support(self.ctx._h, self._h, out.ctypes.data, total, oo.ctypes.data))
        return out[:total], oo

    def strand(self):
        """The strand vote (docs/auto_strand.md) as a STRAND_DTYPE array of one row per read: solid and IN k-mers of the
        read as it came and of its reverse complement, and the orientation chosen.  Runs the vote if the batch has none."""
        _chk(lib().talc_batch_strand(self.ctx._h, self._h))
        rows = np.zeros(self.n_reads, dtype=STRAND_DTYPE)
        _chk(lib().talc_batch_fetch_strand(self.ctx._h, self._h, rows.ctypes.data))
        return rows

    def chimera(self):
        """The chimera scan (docs/chimeras.md): (hits as a CHIMERA_DTYPE array in the order (read, end, adapter, strand),
        read_hit_offsets); on a split batch the hits of the reads it was made from."""
        _chk(lib().talc_batch_chimera(self.ctx._h, self._h))
        n = int(lib().talc_batch_num_chimera_hits(self._h))
        hits = np.zeros(n, dtype=CHIMERA_DTYPE)
        off = np.zeros(self.n_source_reads + 1, dtype=np.uint64)
        _chk(lib().talc_batch_fetch_chimera(self.ctx._h, self._h, hits.ctypes.data, n, off.ctypes.data))
        return hits, off

    def split_pieces(self):
        """Of a split batch: (pieces as a SPLIT_PIECE_DTYPE array, one per read of the batch; read_piece_offsets of the
        source reads)."""
        pieces = np.zeros(int(lib().talc_batch_num_split_pieces(self._h)), dtype=SPLIT_PIECE_DTYPE)
        off = np.zeros(self.n_source_reads + 1, dtype=np.uint64)
        _chk(lib().talc_batch_fetch_split(self.ctx._h, self._h, pieces.ctypes.data, off.ctypes.data))
        return pieces, off

    def demux(self):
        """The barcode calls (docs/demux.md) as a DEMUX_DTYPE array of one row per source read: the reads of a plain or
        clipped batch, the reads a split batch was made from."""
        _chk(lib().talc_batch_demux(self.ctx._h, self._h))
        rows = np.zeros(self.n_source_reads, dtype=DEMUX_DTYPE)
        _chk(lib().talc_batch_fetch_demux(self.ctx._h, self._h, rows.ctypes.data))
        return rows

    def umi(self):
        """The UMI read-out (docs/umi.md) as a UMI_DTYPE array of one row per read of the batch; on a clipped or split
        batch the rows of the scan that made it."""
        _chk(lib().talc_batch_umi(self.ctx._h, self._h))
        rows = np.zeros(self.n_reads, dtype=UMI_DTYPE)
        _chk(lib().talc_batch_fetch_umi(self.ctx._h, self._h, rows.ctypes.data))
        return rows

    def ends(self):
        """The end scan (docs/read_ends.md) as an ENDS_DTYPE array of one row per read; on a clipped batch the rows of the
        reads it was made from."""
        _chk(lib().talc_batch_ends(self.ctx._h, self._h))
        rows = np.zeros(self.n_reads, dtype=ENDS_DTYPE)
        _chk(lib().talc_batch_fetch_ends(self.ctx._h, self._h, rows.ctypes.data))
        return rows

    def pieces(self, mode, min_len=0, soft_mask=False):
        """Trimmed (PIECES_TRIM) or split (PIECES_SPLIT) output of the last correction (docs/trim_split.md; needs
        Context.record_map() before it): (bytes uint8, piece_offsets u64[n_pieces + 1], pieces as a PIECE_DTYPE array,
        read_piece_offsets u64[n_reads + 1]).  Pieces shorter than min_len are dropped; soft_mask: the weak stretches
        inside a trimmed piece in lower case."""
        L = lib()
        _chk(L.talc_batch_pieces(self.ctx._h, self._h, int(mode), int(min_len), 1 if soft_mask else 0))
        n, nb = int(L.talc_batch_num_pieces(self._h)), int(L.talc_batch_pieces_bytes(self._h))
        out = np.empty(max(nb, 1), dtype=np.uint8)
        po = np.empty(n + 1, dtype=np.uint64)
        pc = np.empty(max(n, 1), dtype=PIECE_DTYPE)
        rpo = np.empty(self.n_reads + 1, dtype=np.uint64)
        _chk(L.talc_batch_fetch_pieces(self.ctx._h, self._h, out.ctypes.data, nb, po.ctypes.data, pc.ctypes.data, n, rpo.ctypes.data))
        return out[:nb], po, pc[:n], rpo

    def edits(self, max_cells=0, scratch_bytes=None):
        """The edit scripts of the last correction (docs/correction_edits.md; needs Context.record_map() before it): (ops
        uint32[] — len << 4 | code —, op_offsets u64[n_reads + 1], rows as an EDIT_ROW_DTYPE array).  A CORRECTED segment
        of more than max_cells cells (0: 1 << 26) is not aligned.  scratch_bytes: test hook, another scratch budget."""
        L = lib()
        if scratch_bytes is None:
            _chk(L.talc_batch_edits(self.ctx._h, self._h, int(max_cells)))
        else:
            _chk(L.talc_test_batch_edits(self.ctx._h, self._h, int(max_cells), int(scratch_bytes)))
        n = int(L.talc_batch_num_edit_ops(self._h))
        ops = np.empty(max(n, 1), dtype=np.uint32)
        oo = np.empty(self.n_reads + 1, dtype=np.uint64)
        rows = np.zeros(self.n_reads, dtype=EDIT_ROW_DTYPE)
        _chk(L.talc_batch_fetch_edits(self.ctx._h, self._h, ops.ctypes.data, n, oo.ctypes.data, rows.ctypes.data))
        return ops[:n], oo, rows

    def fetch_read_stats(self):
        """int64[n, 5]: {row written, raw length, IN-region span, IN regions, corrected length} (Read.cpp:418-433)."""
        st = np.zeros((self.n_reads, 5), dtype=np.int64)
        _chk(lib().talc_batch_fetch_read_stats(self.ctx._h, self._h, st.ctypes.data))
        return st

    @property
    def corrected_bytes(self):
        return int(lib().talc_batch_corrected_bytes(self._h))

    def copy_corrected_to_device(self, device_ptr, capacity):
        """Device-to-device copy of the dense corrected records into a caller-owned buffer."""
        oo = np.empty(self.n_reads + 1, dtype=np.uint64)
        st = np.empty(self.n_reads, dtype=np.int32)
        _chk(lib().talc_batch_copy_corrected_device(self.ctx._h, self._h, C.c_void_p(device_ptr), capacity, oo.ctypes.data, st.ctypes.data))
        return oo, st

    def trace(self, read_index):
        cap = 1 << 22
        while True:
            buf = C.create_string_buffer(cap)
            need = lib().talc_batch_trace_read(self.ctx._h, self._h, read_index, buf, cap)
            if need < 0:
                _chk(int(need))
            if need <= cap:
                return buf.value.decode()
            cap = int(need) + 16
