"""Trimmed and split output (docs/trim_split.md) in numpy: the contract of talc_batch_pieces / talc_batch_fetch_pieces
from a correction map and the records it describes.  Nothing here looks at a device result of those calls.

A byte of a record is weak when it lies in a RAW segment, trusted otherwise; segments with out_len 0 hold no byte.
split: the maximal runs of trusted bytes; trim: first trusted byte .. last trusted byte; pieces shorter than min_len are
dropped; pieces are ordered by read, then by out_start."""
import numpy as np

import corr_map_ref as M

TRIM, SPLIT = 1, 2
PIECE_DTYPE = np.dtype([("read", "<u4"), ("out_start", "<u4"), ("out_len", "<u4")])


def read_runs(segs, mode):
    """[(out_start, out_len)] of one read's pieces before min_len, from its segments (SEGMENT_DTYPE rows)."""
    s = segs[segs["out_len"] > 0]                      # empty segments are looked through
    t = s["kind"] != M.RAW
    if not t.any():
        return []
    start, end = s["out_start"].astype(np.int64), s["out_start"].astype(np.int64) + s["out_len"]
    if mode == TRIM:
        i = np.nonzero(t)[0]
        return [(int(start[i[0]]), int(end[i[-1]] - start[i[0]]))]
    d = np.diff(np.concatenate(([0], t.astype(np.int8), [0])))
    first, last = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0] - 1   # the trusted runs among the non-empty segments
    return [(int(start[a]), int(end[b] - start[a])) for a, b in zip(first, last)]


def pieces(segments, seg_offsets, records, record_offsets, mode, min_len=0, masked_records=None):
    """(bytes uint8, piece_offsets u64[n_pieces + 1], pieces PIECE_DTYPE[n_pieces], read_piece_offsets u64[n_reads + 1]).
    masked_records: the records with their RAW bases in lower case; given, a trimmed piece is cut from them."""
    assert mode in (TRIM, SPLIT)
    src = masked_records if (mode == TRIM and masked_records is not None) else records
    n = len(seg_offsets) - 1
    rows, chunks, rpo = [], [], [0]
    for r in range(n):
        base = int(record_offsets[r])
        for a, ln in read_runs(segments[int(seg_offsets[r]):int(seg_offsets[r + 1])], mode):
            if ln >= min_len:
                assert base + a + ln <= int(record_offsets[r + 1])
                rows.append((r, a, ln))
                chunks.append(src[base + a:base + a + ln])
        rpo.append(len(rows))
    pc = np.zeros(len(rows), dtype=PIECE_DTYPE)
    for i, row in enumerate(rows):
        pc[i] = row
    po = np.zeros(len(rows) + 1, dtype=np.uint64)
    po[1:] = np.cumsum(pc["out_len"].astype(np.uint64))
    data = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
    return np.asarray(data, dtype=np.uint8), po, pc, np.asarray(rpo, dtype=np.uint64)


def from_expected(exp):
    """The arguments of pieces() from corr_map_ref.expected() dicts: (segments, seg_offsets, records, record_offsets,
    masked records) — the oracle-trace-derived map and the oracle's records."""
    segs = M.as_array([s for e in exp for s in e["segs"]])
    so = np.cumsum([0] + [len(e["segs"]) for e in exp]).astype(np.uint64)
    ro = np.cumsum([0] + [len(e["out"]) for e in exp]).astype(np.uint64)
    rec = np.frombuffer("".join(e["out"] for e in exp).encode(), dtype=np.uint8)
    msk = np.frombuffer("".join(M.masked(e) for e in exp).encode(), dtype=np.uint8)
    return segs, so, rec, ro, msk


def piece_texts(result):
    """[[str]]: the texts of every read's pieces."""
    data, po, pc, rpo = result
    return [[bytes(data[int(po[i]):int(po[i + 1])]).decode() for i in range(int(rpo[r]), int(rpo[r + 1]))] for r in range(len(rpo) - 1)]


def fasta_lines(names, result, split):
    """The lines of <o>.trim.fa (split False: >name) or <o>.split.fa (>name_1, >name_2, ... over the kept pieces)."""
    out = []
    for name, texts in zip(names, piece_texts(result)):
        for i, t in enumerate(texts):
            out.append(">" + name + ("_%d" % (i + 1) if split else ""))
            out += [t[p:p + 70] for p in range(0, len(t), 70)]
    return out
