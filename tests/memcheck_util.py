"""What the poison tests share (tests/test_gpu_poison.py; the hooks: talc_devmem.h, lib.poisoned): the pattern bytes, every
output of a corrected batch as per-read tuples of bytes and integers, and the guard report's before / after."""
import contextlib

import numpy as np

import parity_util as PU
from talc_amd import lib as T

# 0x00 is the control (what fresh device memory reads as in practice), 0xFF the tables' empty-key fill
PATTERNS = (0x00, 0xFF, 0xA5)
# where a buffer holds text: a parser or counter that reads the pad would extend a count ('5'), a k-mer ('A') or a line
TEXT_PATTERNS = PATTERNS + (0x35, 0x41, 0x0A)

FORWARD = ("records", "masked", "map", "solidity", "support", "pieces", "edits")
BACKWARD = ("edits", "pieces", "support", "solidity", "map", "masked", "records")


def fetch_all(b, order=FORWARD):
    """Every output of the corrected batch b (its context kept the map), requested in `order`."""
    f = {}
    for what in order:
        if what == "records":
            out, f["oo"], f["st"] = b.fetch_corrected()
            f["out"] = bytes(out)
        elif what == "masked":
            f["msk"] = bytes(b.fetch_corrected(soft_mask=True)[0])
        elif what == "map":
            f["segs"], f["so"] = b.fetch_map()
        elif what == "solidity":
            f["raw"], f["cor"] = b.solidity()
        elif what == "support":
            f["support"] = []
            for kw in (dict(source="record"), dict(source="raw"), dict(phred=(2, 40))):
                sb, so = b.support(**kw)
                f["support"].append((bytes(sb), so))
        elif what == "pieces":
            f["pieces"] = []
            for mode, mask in ((T.PIECES_TRIM, True), (T.PIECES_TRIM, False), (T.PIECES_SPLIT, False)):
                pb, po, pc, rpo = b.pieces(mode, 0, mask)
                f["pieces"].append((bytes(pb), po, pc, rpo))
        elif what == "edits":
            f["ops"], f["eo"], f["erows"] = b.edits()
        else:
            raise ValueError(what)
    f["stats"] = b.fetch_read_stats()
    return f


def per_read(f, n, batch_free=False):
    """fetch_all's result as one tuple per read.  batch_free: without the read's number in its batch (talc_piece.read), so
    that a read's tuple is the same in whatever batch it was corrected."""
    out, oo, st, msk, segs, so = f["out"], f["oo"], f["st"], f["msk"], f["segs"], f["so"]
    raw, cor, ops, eo, erows, stats = f["raw"], f["cor"], f["ops"], f["eo"], f["erows"], f["stats"]
    per = []
    for r in range(n):
        rec = (out[int(oo[r]):int(oo[r + 1])], int(st[r]), msk[int(oo[r]):int(oo[r + 1])], segs[int(so[r]):int(so[r + 1])].tobytes(),
               raw[r].tolist(), cor[r].tolist(), ops[int(eo[r]):int(eo[r + 1])].tobytes(), erows[r].tolist(), stats[r].tolist())
        for pb, po, pc, rpo in f["pieces"]:
            a, e = int(rpo[r]), int(rpo[r + 1])
            mine = pc[a:e]
            if batch_free:
                assert (mine["read"] == r).all()
                mine = np.stack([mine["out_start"], mine["out_len"]], axis=1)
            rec += (tuple(pb[int(po[i]):int(po[i + 1])] for i in range(a, e)), mine.tobytes())
        for sb, sof in f["support"]:
            rec += (sb[int(sof[r]):int(sof[r + 1])],)
        per.append(rec)
    return per


def everything(ctx, reads, order=FORWARD, batch_free=False):
    """Everything a corrected batch gives, per read: a list of tuples of bytes and integers."""
    ctx.record_map(True)
    b = ctx.batch(*PU.pack_reads(reads))
    try:
        rc = b.correct()
        t = ctx.timing()
        work = (rc, t.n_trail_steps, t.n_dp_cells, t.n_kmers, t.n_bases, t.n_retried, t.n_failed)
        per = per_read(fetch_all(b, order), len(reads), batch_free)
        return per, work, b.strand() if ctx._auto else None
    finally:
        b.close()
        ctx.record_map(False)


# where per_read() puts what, for the tests that look at one field of a read's tuple (batch_free or not)
F_RECORD, F_STATUS, F_MASKED, F_SEGS, F_SOLIDITY_RAW, F_SOLIDITY_RECORD, F_OPS, F_EDIT_ROW, F_STATS = range(9)
F_SPLIT_TEXTS = 9 + 2 * 2                            # fetch_all's third pieces call: the texts of the read's SPLIT pieces
F_SUPPORT = dict(record=-3, raw=-2, phred=-1)        # fetch_all's three support calls come last


def _field_layout_holds():
    """The constants above against per_read itself, on one made-up read."""
    piece = lambda text: (text, np.array([0, len(text)], np.uint64), np.zeros(1, dtype=[("read", "<u4"), ("out_start", "<u4"), ("out_len", "<u4")]), np.array([0, 1], np.uint64))
    f = dict(out=b"REC", oo=np.array([0, 3], np.uint64), st=[7], msk=b"msk", segs=np.zeros(1, np.uint32), so=np.array([0, 1], np.uint64),
             raw=np.array([[1]]), cor=np.array([[2]]), ops=np.zeros(1, np.uint32), eo=np.array([0, 1], np.uint64), erows=np.array([[3]]),
             stats=np.array([[4]]), pieces=[piece(b"tm"), piece(b"t"), piece(b"split")],
             support=[(b"rc", np.array([0, 2], np.uint64)), (b"rw", np.array([0, 2], np.uint64)), (b"ph", np.array([0, 2], np.uint64))])
    t = per_read(f, 1)[0]
    return (t[F_RECORD], t[F_STATUS], t[F_MASKED], t[F_SOLIDITY_RAW], t[F_SOLIDITY_RECORD], t[F_EDIT_ROW], t[F_STATS], t[F_SPLIT_TEXTS],
            t[F_SUPPORT["record"]], t[F_SUPPORT["raw"]], t[F_SUPPORT["phred"]]) == (b"REC", 7, b"msk", [1], [2], [3], [4], (b"split",), b"rc", b"rw", b"ph")


def first_difference(got, want):
    """(read, fields that differ) of the first read whose tuples differ, or None."""
    for i, (x, y) in enumerate(zip(got, want)):
        if x != y:
            return i, [j for j, (a, b) in enumerate(zip(x, y)) if a != b]
    return None if len(got) == len(want) else (min(len(got), len(want)), ["length"])


@contextlib.contextmanager
def guards_checked():
    """Around a test's device work, contexts closed inside: red zones were checked, and none was found written."""
    before = T.guard_report()
    yield before
    after = T.guard_report()
    assert after["checked"] > before["checked"], (before, after)
    assert after["violations"] == 0, after
