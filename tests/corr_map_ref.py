"""The correction map (docs/correction_map.md) of one read from the oracle's trace alone: the expected talc_segment
records, and the piece of the corrected read each of them stands for.

The trace (OracleTable.trace) lists the IN regions after analyzeINRegions (TR_REGION), every search (TR_SEARCH: location,
direction) and its outcome (TR_RESULT: success, the new LEFT.end and RIGHT.start, the weak sequence).  An INNER search
towards RIGHT opens the next gap, one towards LEFT retries the same gap; a successful INNER result moves regE[g] and
regS[g + 1] and replaces the gap, a successful HEAD result moves regS[0], a successful TAIL result regE[last].  Under -rev
the trace is that of the reverse complement: the segments are flipped.  Nothing of the product is looked at here."""
import numpy as np

TR_REGION, TR_SEARCH, TR_RESULT = 1, 3, 5
HEAD, INNER, TAIL = 0, 1, 2
LEFT, RIGHT = 0, 1
SOLID, CORRECTED, RAW = 0, 1, 2
LETTERS = "SCR"
COMP = str.maketrans("ACGTN", "TGCAN")

SEGMENT_DTYPE = np.dtype([("kind", "<u4"), ("raw_start", "<u4"), ("raw_len", "<u4"), ("out_start", "<u4"), ("out_len", "<u4")])


def dna5(seq):
    return "".join(c if c in "ACGT" else "N" for c in seq.upper())


def revcomp(s):
    return s.translate(COMP)[::-1]


def parse_trace(text):
    """(status, events [(kind, a, b, c, d, s)], OUT)."""
    status, out, ev = None, None, []
    for line in text.split("\n"):
        if line.startswith("STATUS "):
            status = int(line[7:])
        elif line.startswith("OUT "):
            out = line[4:]
        elif line:
            f = line.split(" ", 6)
            ev.append((int(f[0]), int(f[1]), int(f[2]), int(f[3]), int(f[4]), f[6] if len(f) > 6 else ""))
    return status, ev, out


def expected(otab, seq):
    """What the map of `seq` must be: dict(segs [(kind, raw_start, raw_len, out_start, out_len)], pieces [str] — the
    text of every segment in the record —, out = the trace's OUT, status, R, facts).  facts: what the read exercises
    (counts of the conditions the tests ask for)."""
    K, rev = int(otab.p.k), bool(otab.p.reverse)
    L = len(seq)
    status, ev, out = parse_trace(otab.trace(seq))
    facts = dict(corrected=0, zero_corrected=0, zero_raw=0, head_corrected=0, tail_corrected=0, head_long=0, tail_long=0, R=0)
    if status != 0:
        raw = dna5(seq)
        if rev:   # (main.cpp:253 reverse-complements every read, :286 only the corrected ones back)
            raw = revcomp(raw)
        return dict(segs=[(RAW, 0, L, 0, L)], pieces=[raw], out=out, status=status, R=0, facts=facts)
    read = dna5(seq)
    if rev:
        read = revcomp(read)
    regS = [e[1] for e in ev if e[0] == TR_REGION]
    regE = [e[2] for e in ev if e[0] == TR_REGION]
    R = len(regS)
    assert R >= 1
    weak = [None] * R          # weak[g]: what replaced the gap after region g
    head = tail = None
    gap, loc = -1, None
    for kind, a, b, c, d, s in ev:
        if kind == TR_SEARCH:
            loc = a
            if a == INNER and b == RIGHT:
                gap += 1
        elif kind == TR_RESULT:
            assert a == loc
            if not b:
                continue
            if a == INNER:
                regE[gap], regS[gap + 1], weak[gap] = c, d, s
            elif a == HEAD:
                regS[0], head = d, s
            else:
                regE[R - 1], tail = c, s
    segs, pieces = [], []

    def add(kind, rs, rl, text):
        segs.append([kind, rs, rl, 0, len(text)])
        pieces.append(text)

    add(CORRECTED if head is not None else RAW, 0, regS[0], head if head is not None else read[:regS[0]])
    for i in range(R):
        add(SOLID, regS[i], regE[i] + K - regS[i], read[regS[i]:regE[i] + K])
        if i + 1 < R:
            rs = regE[i] + K
            rl = max(0, regS[i + 1] - rs)
            add(CORRECTED if weak[i] is not None else RAW, rs, rl, weak[i] if weak[i] is not None else read[rs:rs + rl])
    ts = regE[R - 1] + K
    add(CORRECTED if tail is not None else RAW, ts, L - ts, tail if tail is not None else read[ts:])
    pos = 0
    for s in segs:
        s[3] = pos
        pos += s[4]
    facts.update(corrected=1, R=R, head_corrected=int(head is not None), tail_corrected=int(tail is not None),
                 head_long=int(segs[0][2] > otab.p.max_border_length), tail_long=int(segs[-1][2] > otab.p.max_border_length),
                 zero_corrected=sum(1 for s in segs[2:-1:2] if s[0] == CORRECTED and s[4] == 0),
                 zero_raw=sum(1 for s in segs[2:-1:2] if s[0] == RAW and s[2] == 0))
    if rev:
        segs = [[k, L - rs - rl, rl, pos - os_ - ol, ol] for k, rs, rl, os_, ol in reversed(segs)]
        pieces = [revcomp(p) for p in reversed(pieces)]
    return dict(segs=[tuple(s) for s in segs], pieces=pieces, out=out, status=status, R=R, facts=facts)


def as_array(segs):
    a = np.zeros(len(segs), dtype=SEGMENT_DTYPE)
    for i, s in enumerate(segs):
        a[i] = s
    return a


def masked(e):
    """The record with its RAW segments in lower case."""
    return "".join(p.lower() if s[0] == RAW else p for s, p in zip(e["segs"], e["pieces"]))


def tsv_lines(name, e):
    """The lines of <o>.map.tsv for one read: segments with both lengths 0 are left out."""
    return ["%s\t%s\t%d\t%d\t%d\t%d" % (name, LETTERS[s[0]], s[1], s[2], s[3], s[4]) for s in e["segs"] if s[2] or s[4]]


def raw_overlaps(segs):
    """Pairs of neighbouring segments that overlap in raw coordinates."""
    return sum(1 for a, b in zip(segs, segs[1:]) if a[1] + a[2] > b[1])


# ---------------------------------------------------------------- the input sets of the map tests, built once per process
SETS = {   # name -> (target k-mers, k, seed, generator settings, parameters, reverse)
    "default": (250_000, 21, 77, None, {}, False),
    "reverse": (250_000, 21, 77, None, dict(reverse=1), True),
    "paralog-maxb4": (250_000, 21, 77, dict(paralog_frac=0.7, paralog_div=0.06), dict(max_nb_competing_paths=4, window_size=7), False),
    "k31": (250_000, 31, 77, None, {}, False),
}
COMB_SETS = ("unique-k21", "branching-k21")
_cache = {}


class MapSet:
    """pair: parity_util.Pair (oracle table + product table, not uploaded); reads: the texts; exp: expected() of each."""

    def __init__(self, pair, reads):
        self.pair, self.reads = pair, reads
        self.exp = [expected(pair.otab, s) for s in reads]
        self.facts = {k: sum(e["facts"][k] for e in self.exp) for k in self.exp[0]["facts"] if k != "R"}
        self.maxR = max(e["R"] for e in self.exp)

    def packed(self):
        import parity_util as PU
        return PU.pack_reads(self.reads)

    def counts(self):
        kinds = [s[0] for e in self.exp for s in e["segs"]]
        return dict(segments=len(kinds), S=kinds.count(SOLID), C=kinds.count(CORRECTED), R=kinds.count(RAW), maxR=self.maxR, **self.facts)


def map_set(name, n=200):
    """One of SETS: reads 0 .. n-1 of its generator (reverse-complemented for the -rev set)."""
    if (name, n) not in _cache:
        import parity_util as PU
        target, k, seed, synth_kw, kw, rev = SETS[name]
        pair = PU.Pair(target_kmers=target, k=k, seed=seed, synth_kw=synth_kw, **kw)
        reads = PU.seqs_of(*pair.reads(0, n))
        if rev:
            reads = [revcomp(s) for s in reads]
        _cache[(name, n)] = MapSet(pair, reads)
    return _cache[(name, n)]


def comb_set(graph, per_kind=6):
    """Comb reads (parity_util.comb: one base in K + g spoilt, so an error-free read becomes a region every few k-mers,
    R > 64) on one of COMB_SETS: error-free reads of 2.5 to 3 kb among the generator's first 120, per_kind of them spoilt
    with N and the same again by substitution; of those, the ones the oracle corrects."""
    if ("comb", graph, per_kind) not in _cache:
        import parity_util as PU
        k, seed, synth_kw = PU.comb_synth_kw(graph)
        pair = PU.Pair(target_kmers=60_000, k=k, seed=seed, synth_kw=synth_kw)
        seqs = [s for s in PU.seqs_of(*pair.synth.reads(0, 120)) if 2500 <= len(s) <= 3000]
        rng = np.random.default_rng(5)
        reads = [PU.comb(s, k, how, rng) for how in ("N", "sub") for s in seqs[:per_kind]]
        m = MapSet(pair, reads)
        keep = [i for i, e in enumerate(m.exp) if e["status"] == 0]
        m.reads, m.exp = [m.reads[i] for i in keep], [m.exp[i] for i in keep]
        _cache[("comb", graph, per_kind)] = m
    return _cache[("comb", graph, per_kind)]
