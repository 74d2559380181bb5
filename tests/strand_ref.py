"""Auto strand's contract (docs/auto_strand.md) in plain numpy: the six integers of talc_strand for one read, from the
table's counts alone — a {packed k-mer: count} dict or Table.lookup_host.  Never from a device result."""
import numpy as np

import solidity_ref as S

FIELDS = ("n_kmers", "fwd_solid", "fwd_in", "rc_solid", "rc_in", "reverse")
DTYPE = np.dtype([(f, "<u4") for f in FIELDS])


def choose(fwd_solid, fwd_in, rc_solid, rc_in):
    """The decision rule: 1 iff rc_in > fwd_in, or rc_in == fwd_in and rc_solid > fwd_solid."""
    return 1 if (rc_in > fwd_in or (rc_in == fwd_in and rc_solid > fwd_solid)) else 0


def revcomp_packed(km, k):
    """The reverse complement of packed k-mers (uint64, first base most significant)."""
    km = np.asarray(km, dtype=np.uint64)
    out = np.zeros(len(km), dtype=np.uint64)
    x = ~km
    for _ in range(k):
        out = (out << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return out


def both_counts(raw, k, lookup):
    """(f, r): f[i] the table count of S[i, i + k), r[i] that of its reverse complement, S = dna5(raw); 0 when the
    k-mer is absent or holds an N."""
    km, bad = S.kmers_of(S.dna5(raw), k)
    f = np.zeros(len(km), dtype=np.uint32)
    r = np.zeros(len(km), dtype=np.uint32)
    if (~bad).any():
        f[~bad] = lookup(km[~bad])
        r[~bad] = lookup(revcomp_packed(km[~bad], k))
    return f, r


def row(raw, k, minc, lookup):
    f, r = both_counts(raw, k, lookup)
    fs, fi, rs, ri = int((f >= minc).sum()), int((f > minc).sum()), int((r >= minc).sum()), int((r > minc).sum())
    return (len(f), fs, fi, rs, ri, choose(fs, fi, rs, ri))


def rows(reads, k, minc, lookup):
    """One DTYPE record per read (raw bytes as text: lower case and other letters as they come)."""
    out = np.zeros(len(reads), dtype=DTYPE)
    for i, s in enumerate(reads):
        out[i] = row(s, k, minc, lookup)
    return out


def brute_row(raw, k, minc, table):
    """The same six integers by loops over positions and bases, from a {packed k-mer: count} dict."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    s = "".join(ch.upper() if ch in "ACGTacgt" else "N" for ch in raw)
    n = max(0, len(s) - k + 1)
    fs = fi = rs = ri = 0
    for i in range(n):
        w = s[i:i + k]
        if "N" in w:
            continue
        f = table.get(S.pack(w), 0)
        r = table.get(S.pack("".join(comp[ch] for ch in reversed(w))), 0)
        fs += f >= minc
        fi += f > minc
        rs += r >= minc
        ri += r > minc
    rev = 0
    if ri > fi:
        rev = 1
    elif ri == fi and rs > fs:
        rev = 1
    return (n, fs, fi, rs, ri, rev)
