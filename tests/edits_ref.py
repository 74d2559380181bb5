"""The edit scripts of a correction (docs/correction_edits.md) in numpy: the contract of talc_batch_edits /
talc_batch_fetch_edits from the reads, a correction map and the records it describes.  Nothing here looks at a device result
of those calls.

The script of a read is, segment by segment: out_len '=' for a SOLID or RAW segment (nothing is compared); for a CORRECTED
segment raw_len D when the record side is empty, out_len I when the raw side is, raw_len D then out_len I when raw_len *
out_len > max_cells (the segment is unaligned), else the canonical optimal unit-cost alignment: from the far corner take the
diagonal when it is optimal, else D when that is optimal, else I.  Equal neighbours are merged over the whole read."""
import numpy as np

import corr_map_ref as M

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8          # BAM's codes
LETTER = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
DEFAULT_MAX_CELLS = 1 << 26
EDIT_ROW_DTYPE = np.dtype([(f, "<u4") for f in ("n_match", "n_mismatch", "n_ins", "n_del", "n_ops", "n_unaligned")])


def dna5_bytes(seq):
    """A read (str, bytes or uint8 array) as the correction sees its bytes: upper case, anything but ACGT an N."""
    a = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8) & 0xDF
    return np.where(np.isin(a, np.frombuffer(b"ACGT", dtype=np.uint8)), a, ord("N")).astype(np.uint8)


def matrix(a, b):
    """D[i][j] = the edit distance of a[:i] and b[:j], row by row: the minimum over the row's horizontal moves is a
    running minimum of (value - column)."""
    n, m = len(a), len(b)
    D = np.zeros((n + 1, m + 1), dtype=np.int32)
    cols = np.arange(m + 1, dtype=np.int32)
    D[0] = cols
    for i in range(1, n + 1):
        t = np.empty(m + 1, dtype=np.int32)
        t[0] = i
        np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (b != a[i - 1]), out=t[1:])
        D[i] = np.minimum.accumulate(t - cols) + cols
    return D


_aligned = {}   # (a, b) -> align(a, b): the same pairs come back under another max_cells


def align(a, b):
    """([(code, len)] merged, distance) of the canonical alignment of two non-empty uint8 arrays."""
    key = (a.tobytes(), b.tobytes())
    if key not in _aligned:
        _aligned[key] = _align(a, b)
    return _aligned[key]


def _align(a, b):
    D = matrix(a, b)
    i, j = len(a), len(b)
    ops = []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1, j - 1] + (a[i - 1] != b[j - 1]) == D[i, j]:
            ops.append(OP_EQ if a[i - 1] == b[j - 1] else OP_X)
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1, j] + 1 == D[i, j]:
            ops.append(OP_D)
            i -= 1
        else:
            assert j > 0 and D[i, j - 1] + 1 == D[i, j]
            ops.append(OP_I)
            j -= 1
    return merge([(c, 1) for c in reversed(ops)]), int(D[len(a), len(b)])


def merge(runs):
    out = []
    for c, ln in runs:
        if ln == 0:
            continue
        if out and out[-1][0] == c:
            out[-1] = (c, out[-1][1] + ln)
        else:
            out.append((c, ln))
    return out


def part(a, b, max_cells):
    """([(code, len)], unaligned) of a CORRECTED segment."""
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return merge([(OP_D, n), (OP_I, m)]), 0
    if n * m > max_cells:
        return [(OP_D, n), (OP_I, m)], 1
    return align(a, b)[0], 0


def read_script(raw, segs, rec, max_cells):
    """([(code, len)] merged, n_unaligned) of one read: raw and rec uint8 arrays, segs SEGMENT_DTYPE rows."""
    runs, unal = [], 0
    for s in segs:
        if s["kind"] != M.CORRECTED:
            runs.append((OP_EQ, int(s["out_len"])))
            continue
        p, u = part(raw[int(s["raw_start"]):int(s["raw_start"]) + int(s["raw_len"])], rec[int(s["out_start"]):int(s["out_start"]) + int(s["out_len"])], max_cells)
        runs += p
        unal += u
    return merge(runs), unal


def edits(reads, segments, seg_offsets, records, record_offsets, max_cells=0):
    """(ops uint32[], op_offsets u64[n_reads + 1], rows EDIT_ROW_DTYPE[n_reads]).  reads: the texts as the caller gave
    them; records: uint8, concatenated."""
    max_cells = max_cells or DEFAULT_MAX_CELLS
    n = len(reads)
    assert len(seg_offsets) == n + 1 and len(record_offsets) == n + 1
    ops, oo = [], [0]
    rows = np.zeros(n, dtype=EDIT_ROW_DTYPE)
    for r in range(n):
        rec = np.asarray(records[int(record_offsets[r]):int(record_offsets[r + 1])], dtype=np.uint8)
        runs, unal = read_script(dna5_bytes(reads[r]), segments[int(seg_offsets[r]):int(seg_offsets[r + 1])], rec, max_cells)
        by = {c: sum(ln for k, ln in runs if k == c) for c in LETTER}
        rows[r] = (by[OP_EQ], by[OP_X], by[OP_I], by[OP_D], len(runs), unal)
        ops += [(ln << 4) | c for c, ln in runs]
        oo.append(len(ops))
    return np.asarray(ops, dtype=np.uint32), np.asarray(oo, dtype=np.uint64), rows


def pair_ops(a, b, max_cells=0):
    """The ops (uint32[]) of one pair of texts as one CORRECTED segment, compared byte for byte as given."""
    x, y = (np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8) for s in (a, b))
    return np.asarray([(ln << 4) | c for c, ln in part(x, y, max_cells or DEFAULT_MAX_CELLS)[0]], dtype=np.uint32)


def cigar_text(ops):
    return "".join("%d%s" % (int(o) >> 4, LETTER[int(o) & 15]) for o in ops) or "*"


def apply(ops, raw):
    """The record a script makes of `raw` (uint8 array) — X and I bases are unknown, so: (length, [(raw index | -1)])."""
    i, src = 0, []
    for o in ops:
        ln, c = int(o) >> 4, int(o) & 15
        if c in (OP_EQ, OP_X):
            src += [(c, k) for k in range(i, i + ln)]
            i += ln
        elif c == OP_D:
            i += ln
        else:
            src += [(c, -1)] * ln
    return i, src


def tsv_lines(names, reads, statuses, record_offsets, result, as_seen):
    """The lines of <o>.edits.tsv after the header: as_seen[r] True when the record is in the orientation the correction
    worked in rather than the caller's."""
    ops, oo, rows = result
    out = []
    for r, name in enumerate(names):
        w = rows[r]
        out.append("\t".join([name, str(int(statuses[r])), str(len(reads[r])), str(int(record_offsets[r + 1]) - int(record_offsets[r])),
                              str(int(w["n_match"])), str(int(w["n_mismatch"])), str(int(w["n_ins"])), str(int(w["n_del"])), str(int(w["n_unaligned"])),
                              "-" if as_seen[r] else "+", cigar_text(ops[int(oo[r]):int(oo[r + 1])])]))
    return out
