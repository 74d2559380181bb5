"""The long-read preparation options together (docs/read_preparation.md): the four contracts of tests/ends_ref.py,
chimera_ref.py, demux_ref.py and umi_ref.py composed in the order the library runs them, in numpy and plain Python alone
(never from a device result).  chain() says what a batch of each kind must hold under any legal subset of the settings;
dress() and reads_of() make the molecules the composition is tried on.  tests/test_prep_reference.py holds chain() against
the steps done by hand, the GPU tests hold the device against chain()."""
import numpy as np

import chimera_ref as CR
import demux_ref as DR
import ends_ref as R
import umi_ref as U

SSP23 = CR.SSP[:23]                                   # the strand-switch primer up to where the UMI begins
VNP = CR.VNP
BC24 = DR.barcode_set(96, 24, seed=11, min_dist=9)

# the settings used throughout
ENDS_KW = dict(adapters=[SSP23, VNP], max_error_pct=20, poly_min=12, window=512)
CHIMERA = (True, 10, 100)                             # on, max_error_pct, min_piece
DEMUX = (BC24, 20, 2)                                 # barcodes, max_error_pct, min_margin
UMI = (U.BARE + "GGG", 10, 256)                       # pattern, max_error_pct, window

KINDS = (("plain", False, False), ("clip", True, False), ("split", False, True), ("split + clip", True, True))   # name, clip, split


# ------------------------------------------------------------------ the molecules
def dress(rng, body, barcode):
    """barcode' . junk . SSP23 . umi' . GGG . body . A{15..39} . revcomp(VNP) . junk . revcomp(barcode''), or the reverse
    complement of all of it; the barcode copies and the UMI carry 0 to 2 edits each."""
    junk = lambda: R.random_seq(rng, int(rng.integers(0, 11)))
    copy = lambda: R.mutate(rng, barcode, int(rng.integers(0, 3)), "SID")
    umi = R.mutate(rng, U.instance(rng, U.BARE), int(rng.integers(0, 3)), "SID")
    s = copy() + junk() + SSP23 + umi + "GGG" + body + "A" * int(rng.integers(15, 40)) + R.revcomp(VNP).decode() + junk() + R.revcomp(copy()).decode()
    return s if rng.integers(2) else R.revcomp(s).decode()


def edge_reads(rng):
    """"", a read shorter than every pattern, one of which nothing is left after the clip, one bare barcode."""
    return ["", "ACGT", SSP23 + U.instance(rng, U.BARE) + "GGG", BC24[int(rng.integers(96))]]


def reads_of(bodies, rng):
    """Every body dressed with a random barcode of BC24, those with index i % 9 == 4 left as they are; every tenth read
    joined to the next through chimera_ref.joint; the four edge reads behind them."""
    one = [R.as_bytes(b).decode() if i % 9 == 4 else dress(rng, R.as_bytes(b).decode(), BC24[int(rng.integers(96))]) for i, b in enumerate(bodies)]
    reads, i = [], 0
    while i < len(one):
        if i % 10 == 9 and i + 1 < len(one):
            reads.append(one[i] + CR.joint(rng) + one[i + 1])
            i += 2
        else:
            reads.append(one[i])
            i += 1
    return reads + edge_reads(rng)


# ------------------------------------------------------------------ the composition
_memo = {}


def _once(name, fn, reads, *args):
    """fn(reads, *args) of the reference modules under `name`, computed once per input (the GPU tests ask for the same rows
    under many subsets of the settings); the result is shared and left unchanged."""
    key = (name, tuple(reads), repr(args))
    if key not in _memo:
        _memo[key] = fn(reads, *args)
    return _memo[key]


def _ends_rows(reads, kw):
    return _once("ends", lambda r, a, e, p, w: R.rows(r, adapters=a, max_error_pct=e, poly_min=p, window=w), reads, list(kw.get("adapters", ())),
                 kw.get("max_error_pct", 20), kw.get("poly_min", 0), kw.get("window", R.DEFAULT_WINDOW))


def _umi_rows(reads, umi, claims):
    return _once("umi", lambda r, p, e, w, c: U.rows(r, p, e, w, claims=c), reads, umi[0], umi[1], umi[2] if len(umi) > 2 else U.DEFAULT_WINDOW, claims)


def chain(reads, ends_kw=None, chimera=None, demux=None, umi=None, clip=False, split=False):
    """What a batch of `reads` (str) made with clip / split must hold on a context with the given settings (None: off), in
    the order of docs/umi.md ("Clipping") and docs/demux.md ("Calls"):

      demux      the rows of the reads as they came, whatever the batch kind; None when demux is off
      hits, hit_off    the chimera hits of the reads as they came; None when the scan is off or has no adapter, and on a
                 clipped batch that is not split (it no longer holds the reads as they came)
      pieces, piece_off    of a split batch; else None
      came       the batch's reads before any clipping: the reads, or the pieces of a split batch
      ends       the end rows of `came`; None when the ends are off
      umi        the UMI rows of `came`: with the end rows' claims exactly when the batch is clipped and the ends are on,
                 else by the plain formula; None when the UMI is off
      texts      what the batch's reads must equal: `came`, cut at the UMI rows' intervals (or the end rows', with the UMI
                 off) when the batch is clipped
    """
    reads = [R.as_bytes(r).decode("latin-1") for r in reads]
    adapters = list(ends_kw.get("adapters", ())) if ends_kw else []
    scan = bool(chimera and chimera[0] and adapters)
    assert not split or scan, "a split needs the chimera scan and an adapter"
    assert not clip or ends_kw or umi, "a clip needs the ends or the UMI"
    out = dict.fromkeys(("demux", "hits", "hit_off", "pieces", "piece_off", "ends", "umi"))
    if demux:
        out["demux"] = _once("demux", DR.rows, reads, *demux)
    came = reads
    if scan and (split or not clip):
        out["hits"], out["hit_off"] = _once("hits", CR.hits, reads, adapters, chimera[1])
    if split:
        out["pieces"], out["piece_off"] = CR.pieces([len(x) for x in reads], out["hits"], chimera[2])[:2]
        came = [x.decode("latin-1") for x in CR.cut(reads, out["pieces"])]
    if ends_kw:
        out["ends"] = _ends_rows(came, ends_kw)
    if umi:
        out["umi"] = _umi_rows(came, umi, U.claims_of(out["ends"]) if clip and ends_kw else None)
    texts = came
    if clip:
        texts = [x.decode("latin-1") for x in (U.clip(came, out["umi"]) if umi else R.clip(came, out["ends"]))]
    out.update(came=came, texts=texts)
    return out


def legal(ends_on, chimera_on, umi_on, clip, split):
    """Whether the library makes a batch of this kind on a context with these settings."""
    return (not split or (chimera_on and ends_on)) and (not clip or ends_on or umi_on)


def subsets():
    """Every legal subset of the four settings as (ends, chimera, demux, umi) of booleans: chimera only with the ends."""
    return [(e, c, d, u) for e in (True, False) for c in (True, False) for d in (True, False) for u in (True, False) if e or not c]
