"""The both-strands contract in numpy (docs/both_strands.md): the reference the GPU fold is tested against.

rc(x) is the reverse complement of a packed k-mer (2 bits per base, A=0 C=1 G=2 T=3, first base most significant);
canon(x) = min(x, rc(x)) as unsigned integers, which is lexicographic with A<C<G<T (Jellyfish's -C).  The folded count
C(y) of a canonical k-mer y is the sum of the counts of every observation whose canonical form is y: a window of a read
counts once (a palindromic window too), an entry (x, c) adds c to C(canon(x)), entries of the same k-mer add up, a count
of 0 adds nothing.  The table stores y and rc(y) with C(y) for every y with C(y) >= MIN_COUNT, a palindrome once."""
import collections

import numpy as np

import kmer_ref as R


def rc(kmers, k):
    """Reverse complement of packed k-mers (u64 array or int)."""
    x = np.asarray(kmers, dtype=np.uint64)
    out = np.zeros_like(x)
    for _ in range(k):
        out = (out << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x = x >> np.uint64(2)
    return out


def canon(kmers, k):
    x = np.asarray(kmers, dtype=np.uint64)
    return np.minimum(x, rc(x, k))


def is_palindrome(kmers, k):
    x = np.asarray(kmers, dtype=np.uint64)
    return x == rc(x, k)


def fold(kmers, counts, k):
    """(canonical k-mers u64 sorted, folded counts u64) of the entries (kmers[i], counts[i]); entries that add nothing (a
    zero count) claim nothing.  The sums are exact (u64): the caller decides what 32 bits hold."""
    kmers = np.asarray(kmers, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint64)
    keep = counts > 0
    y = canon(kmers[keep], k)
    u, inv = np.unique(y, return_inverse=True)
    s = np.zeros(len(u), dtype=np.uint64)
    np.add.at(s, inv, counts[keep])
    return u, s


def fold_records(bases, offsets, k):
    """fold() of every window of the records (kmer_ref.count's contract: a window counts once, palindromic or not)."""
    km, ct = R.count(bases, offsets, k)
    return fold(km, ct, k)


def expand(ykmers, ycounts, k, min_count=1):
    """(kmers u64 sorted, counts u32): what the table stores: y and rc(y) for every canonical y with C(y) >= min_count, a
    palindrome once.  Every stored k-mer is listed once, with its folded count."""
    y = np.asarray(ykmers, dtype=np.uint64)
    c = np.asarray(ycounts, dtype=np.uint64)
    keep = c >= min_count
    y, c = y[keep], c[keep]
    assert (c <= 0xFFFFFFFF).all(), "a folded count passes 32 bits: the counter refuses it"
    r = rc(y, k)
    twin = r != y
    km = np.concatenate([y, r[twin]])
    ct = np.concatenate([c, c[twin]]).astype(np.uint32)
    o = np.argsort(km, kind="stable")
    return km[o], ct[o]


# ------------------------------------------------------------------ the naive restatement (the self-check of the above)
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp_text(s):
    """Reverse complement of a record; a byte that is no base stays what it is (it breaks the same windows)."""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}
    return "".join(comp.get(ch, ch) for ch in reversed(s))


def naive_fold(records, k):
    """collections.Counter of canonical k-mers (as text, compared as text: lexicographic, A<C<G<T), window by window."""
    out = collections.Counter()
    for r in records:
        r = r.decode("latin-1") if isinstance(r, (bytes, bytearray)) else r
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if all(ch in "ACGTacgt" for ch in w):
                w = w.upper()
                m = "".join(_COMP[ch] for ch in reversed(w))
                out[min(w, m)] += 1
    return out


def pack_text(s):
    x = 0
    for ch in s:
        x = (x << 2) | "ACGT".index(ch)
    return x


def palindrome_records(k, n=6, seed=11):
    """Records h + revcomp(h) with len(h) >= k / 2 + 3: for even k they hold the palindromic k-mer centred on the seam."""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        h = "".join(rng.choice(list("ACGT"), size=k // 2 + 3 + i))
        recs.append(h + revcomp_text(h))
    recs.append(recs[0])    # the same palindrome a second time
    return recs


def flip_records(bases, offsets, rng):
    """The records, each reverse-complemented with probability 1/2 (one rng.random(n) draw); the same offsets."""
    bases = np.asarray(bases, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    lut = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        lut[a] = b
    flip = rng.random(len(offsets) - 1) < 0.5
    out = bases.copy()
    lens = np.diff(offsets)
    if len(set(lens.tolist())) == 1 and len(lens):     # equal lengths: one reshape
        L = int(lens[0])
        m = out[offsets[0]:offsets[-1]].reshape(-1, L)
        m[flip] = lut[m[flip][:, ::-1]]
    else:
        for i in np.nonzero(flip)[0]:
            a, b = int(offsets[i]), int(offsets[i + 1])
            out[a:b] = lut[bases[a:b][::-1]]
    return out, flip
