"""The per-base support's contract (docs/base_support.md) in plain numpy: cover, span and the Phred byte of every base of
one sequence, from the table's counts alone — a {packed k-mer: count} dict or Table.lookup_host, through solidity_ref.
Never from a device result."""
import numpy as np

import solidity_ref as S


def span(L, k):
    """span[j]: the k-mer positions whose k-mer holds base j, [max(0, j - k + 1), min(j, n - 1)]; 0 when n = 0."""
    n = max(0, L - k + 1)
    j = np.arange(L, dtype=np.int64)
    if n == 0:
        return np.zeros(L, dtype=np.int64)
    return np.minimum(j, n - 1) - np.maximum(0, j - k + 1) + 1


def cover_of_counts(c, L, k, minc):
    """cover[j]: the solid positions among those span[j] counts."""
    n = len(c)
    assert n == max(0, L - k + 1)
    pre = np.concatenate([[0], np.cumsum(np.asarray(c) >= minc)]).astype(np.int64)   # pre[i] = solid positions below i
    j = np.arange(L, dtype=np.int64)
    if n == 0:
        return np.zeros(L, dtype=np.int64)
    lo, hi = np.maximum(0, j - k + 1), np.minimum(j, n - 1)
    return pre[hi + 1] - pre[lo]


def cover(seq, k, minc, lookup):
    return cover_of_counts(S.counts(seq, k, lookup), len(seq), k, minc)


def phred_of(cov, spn, qmin, qmax):
    """The quality character: 33 + qmin + (qmax - qmin) * cover // span, 33 + qmin where span is 0."""
    assert 0 <= qmin <= qmax <= 93
    cov, spn = np.asarray(cov, dtype=np.int64), np.asarray(spn, dtype=np.int64)
    q = np.zeros(len(cov), dtype=np.int64)
    has = spn > 0
    q[has] = ((qmax - qmin) * cov[has]) // spn[has]
    return (33 + qmin + q).astype(np.uint8)


def bytes_of(seq, k, minc, lookup, phred=None):
    """One uint8 per base of seq: cover, or with phred=(qmin, qmax) the quality character."""
    cov = cover(seq, k, minc, lookup)
    if phred is None:
        return cov.astype(np.uint8)
    return phred_of(cov, span(len(seq), k), *phred)


def brute(seq, k, minc, table, phred=None):
    """The same bytes by a double loop over bases and k-mer positions, from a {packed k-mer: count} dict."""
    L = len(seq)
    n = max(0, L - k + 1)
    solid = []
    for i in range(n):
        w = seq[i:i + k]
        solid.append((0 if any(ch not in "ACGT" for ch in w) else table.get(S.pack(w), 0)) >= minc)
    out = []
    for j in range(L):
        cov = spn = 0
        for i in range(n):
            if i <= j < i + k:
                spn += 1
                cov += 1 if solid[i] else 0
        if phred is None:
            out.append(cov)
        else:
            out.append(33 + phred[0] + (((phred[1] - phred[0]) * cov) // spn if spn else 0))
    return np.array(out, dtype=np.uint8)


def parse_fastq(text):
    """[(name, sequence, qualities)] of four-line records; asserts the form."""
    lines = text.split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0, "a FASTQ file is four lines per record, each ended by a newline"
    recs = []
    for i in range(0, len(lines) - 1, 4):
        h, s, p, q = lines[i:i + 4]
        assert h.startswith("@") and p == "+" and len(s) == len(q), (i, h)
        recs.append((h[1:], s, q))
    return recs


def parse_fasta(text):
    """[(name, sequence unwrapped)]."""
    recs = []
    for line in text.split("\n"):
        if line.startswith(">"):
            recs.append([line[1:], ""])
        elif line:
            recs[-1][1] += line
    return [(a, b) for a, b in recs]
