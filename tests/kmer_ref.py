"""The k-mer counting contract in numpy (docs/kmer_counting.md): the reference the GPU counter is tested against.

In every record every window of K consecutive bytes that are all one of ACGTacgt counts once; any other byte ends the
window; windows never span two records.  k-mers are directional, 2 bits per base (A=0 C=1 G=2 T=3), first base most
significant."""
import collections

import numpy as np

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[_ch + 32] = _i      # lower case


# hand-made records: shorter than K, exactly K, N / IUPAC / CR inside, lower case, record boundaries, homopolymers
HAND = [
    "",
    "ACGT",
    "ACGTACGTACGTACGTAC",                                   # 18
    "ACGTACGTACGTACGTACGTACGTACGTACG",                      # 31
    "acgtacgtacgtACGTACGTACGTacgtacgtacgTTTG",
    "AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA",
    "ACGTTGCAACGTTGCAACGTNACGTTGCAACGTTGCAACGTTGCAAC",
    "GGGCCCAAATTTGGGCCCAAATTTRGGGCCCAAATTTGGGCCCAAATTTYCC",
    "CCGGAATTCCGGAATTCCGGAATT\rCCGGAATTCCGGAATTCCGGAATTCCGG",
    "TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT",
    "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT",
]


def hand_records():
    rng = np.random.default_rng(5)
    recs = list(HAND)
    for _ in range(40):   # random records with a few breaking bytes, a small alphabet so that k-mers repeat
        n = int(rng.integers(0, 90))
        r = "".join(rng.choice(list("ACGTACGTACGTacgtNRn"), size=n))
        recs.append(r)
    recs.append(HAND[5] + HAND[9])       # a record that ends one homopolymer run and starts another
    return recs


def records_to_arrays(records):
    """(bases uint8, offsets u64[n+1]) of a list of str / bytes records."""
    recs = [r.encode() if isinstance(r, str) else bytes(r) for r in records]
    offsets = np.zeros(len(recs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in recs]) if recs else []
    return np.frombuffer(b"".join(recs), dtype=np.uint8).copy(), offsets


def joined(bases, offsets):
    bases = np.asarray(bases, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    n = len(offsets) - 1
    lens = np.diff(offsets)
    out = np.full(int(lens.sum()) + n, ord("\n"), dtype=np.uint8)
    rec = np.repeat(np.arange(n), lens)                 # record of every byte
    out[np.arange(int(lens.sum())) + rec] = bases[offsets[0]:offsets[-1]]
    return out


def count(bases, offsets, k):
    """(kmers u64 sorted, counts u32) of every valid window of the records."""
    text = joined(bases, offsets)
    n = len(text)
    if n < k:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
    codes = _CODE[text]
    cs = np.concatenate([[0], np.cumsum(codes == 4, dtype=np.int64)])
    nw = n - k + 1
    valid = (cs[k:k + nw] - cs[:nw]) == 0            # window [s, s + k) holds no breaking byte
    c = (codes & 3).astype(np.uint64)
    km = np.zeros(nw, dtype=np.uint64)
    for j in range(k):
        km = (km << np.uint64(2)) | c[j:j + nw]
    u, cnt = np.unique(km[valid], return_counts=True)
    return u, cnt.astype(np.uint32)


def naive_count(records, k):
    """collections.Counter over the records, window by window (the self-check of count())."""
    val = {"A": 0, "C": 1, "G": 2, "T": 3}
    out = collections.Counter()
    for r in records:
        r = r.decode("latin-1") if isinstance(r, (bytes, bytearray)) else r
        for i in range(len(r) - k + 1):
            w = r[i:i + k]
            if all(ch in "ACGTacgt" for ch in w):
                x = 0
                for ch in w.upper():
                    x = (x << 2) | val[ch]
                out[x] += 1
    return out


def unpack(km, k):
    return "".join("ACGT"[(int(km) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def write_dump(path, kmers, counts, k):
    """`jellyfish dump -c` text: 'KMER count' per line."""
    kmers = np.asarray(kmers, dtype=np.uint64)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    chars = np.empty((len(kmers), k + 1), dtype=np.uint8)
    for j in range(k):
        chars[:, j] = letters[((kmers >> np.uint64(2 * (k - 1 - j))) & np.uint64(3)).astype(np.int64)]
    chars[:, k] = ord(" ")
    with open(path, "wb") as f:
        f.write(b"".join(row.tobytes() + b"%d\n" % c for row, c in zip(chars, np.asarray(counts).tolist())))
