"""Reads whose inner gaps take k_search over the sizes at which it changes what it does ("Switch points of
the path search"), and reads beyond 65 535 bases.  Nothing here needs the product or a GPU:
tests/test_long_gap_reference.py asserts from the oracle alone that every case gets where its name says,
tests/test_gpu_long_gaps.py runs them through the HIP path.

A gap read is a random transcript — clean flanks with the gaps' true sequences between them — whose gaps carry a *comb*:
one edit every `period` bases (15, below the smallest K, so no k-mer of a gap is solid at any K and identity stays around
93 %), the gap's first and last base among them.  Substitution comb: the read's gap is as long as the true path.
Deletion comb: shorter by a 15th.  Insertion comb: longer, with period 20 at K = 21 (a bridge is accepted only if it is
less than 5 % shorter than the stretch it replaces, Explorer.cpp:973).  All k-mer counts are equal, so each side of a gap
has one anchor: the flank's k-mer next to the gap.

With a read gap of G bases that starts at read position S, between flanks of FL and FR bases, the regions around it are
[S - FL, S - K] and [S + G, S + G + FR - K], the search from the left anchor starts at whichStart = S - K, and
(talc_kernels_search.h, search_bridge; Explorer.cpp:916-936)

    gapLen  = Rs - (whichStart + K)          = G
    refLen  = Re + K - whichStart            = G + FR + K      (anchor, gap, the whole target region)
    pathMax = int(1.2 * gapLen + 3 * K)

— ref_len() and path_max() below; the CPU file checks them against the oracle's structure and trace (a Trail of
K + step bases ends when it has reached the aim and is longer than refLen; one that finds no aim walks pathMax steps),
the GPU file against the device trace.

A variant site is a second transcript, the 2 K - 1 bases around one base of the gap with another base there: both alleles
have the same count, so a search has two Trails from the step that adds the site.  Trails are scored only on a step that
check_interval divides and only when there are more of them than max_nb_competing_paths (Explorer.cpp:596), and
gardening then keeps every Trail that is first both by score and by distance.  So the two-Trail cases run with
max_nb_competing_paths = 1, and a site sits on a tooth of the comb where the read has *neither* allele: the two Trails tie at
every check and both live on.  (A read that has one of the alleles loses the other Trail at the first check; with the
default limit of 7, two Trails are never scored at all.)  A repeat is a stretch of K + 20 bases of the gap copied to a
second place in it."""
import numpy as np

K_DEFAULT = 21
FLANK = 400
ROW_MAX_REF = 8191                       # talc_kernels_search.h
ROW_COV_LIMIT = 1 << 13                  # 1 << ROW_COV_BITS
ROW_ARENA_INTS = 448 * 1024
NBUF = 576
WIDE_BLOOM_MIN_PATH = 600
WIDE_BLOOM_WORDS = 16384
INSTANCES = (2, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128)      # score_bridges_rows<N>: B = (refLen + 63) / 64 <= N


def ref_len(read_gap, flank_r, k):
    return read_gap + flank_r + k


def path_max(read_gap, k):
    return int(1.2 * read_gap + 3 * k)


def instance_of(ref):
    """N of the score_bridges_rows<N> that scores a search with kept rows at this reference length (score_bridges)."""
    b = (ref + 63) >> 6
    return next((n for n in INSTANCES if b <= n), 0) if ref <= ROW_MAX_REF else 0


def row_records(ref):
    """Records the row arena holds at a reference length (rows_shape): 0 beyond ROW_MAX_REF."""
    if ref > ROW_MAX_REF:
        return 0
    return min(NBUF, ROW_ARENA_INTS // ((ref + 2 + 3) & ~3))


def first_pass_buffers(pmax, k, longest_read):
    """Trail buffers of a first-pass search (make_caps, pool_shape) in a batch whose longest read has that many bases."""
    seq_cap = (int(1.2 * longest_read) + 4 * k + 64 + 15) & ~15
    arena = min(NBUF * seq_cap, max(1 << 20, 8 * seq_cap))
    stride = (k + pmax + 16 + 15) & ~15
    return min(NBUF, arena // stride)


def wide_bloom_words(pmax):
    """0: the cycle filter in LDS alone; else the words of the wide one (init_first_trail)."""
    if pmax <= WIDE_BLOOM_MIN_PATH:
        return 0
    words = 1024
    while words < WIDE_BLOOM_WORDS and words < pmax // 2:
        words <<= 1
    return words


def gap_with_path_max(limit, k, above):
    """The read gap with the largest pathMax <= limit, or (above) the smallest pathMax > limit."""
    g = int((limit - 3 * k) / 1.2) - 3
    while path_max(g + 1, k) <= limit:
        g += 1
    return g + 1 if above else g


def _other(b, rng, also=None):
    rest = [c for c in "ACGT" if c != b and c != also]
    return rest[int(rng.integers(0, len(rest)))]


class Gap:
    """One gap of a GapRead: comb, start (read position of its first base), read_gap, true_len, true_start (position in
    the truth), flank_r (bases of the region after it), sites and repeats (offsets in the true gap), ref_len, path_max."""


class GapRead:
    """What gap_read() / multi_gap_read() return: transcripts (for parity_util.CustomPair), read, truth, k, gaps (Gap
    objects), regions (start and end k-mer position of every solid region).  For a read with one gap the Gap's facts are
    the GapRead's too."""


def multi_gap_read(gaps, k=K_DEFAULT, seed=1, flanks=None):
    """gaps: one dict per gap of true_len and, optionally, comb ("sub" / "del" / "ins"), period, sites, repeats.
    flanks: the clean stretches around them (len(gaps) + 1 lengths; FLANK each by default).
    sites: offsets in the true gap of biallelic sites, each on a tooth of the comb (a multiple of the period) and at
    least K apart; the read has a third base there (in every comb: that tooth is a substitution).  decisive: offsets of
    biallelic sites between two teeth, where the read has the transcript's allele: the Trails double there and the next
    scoring must drop exactly those with the other allele — the one place where a score decides what the trace shows.
    repeats: (from, to) offsets — the K + 20 bases at `from` are copied to `to`."""
    flanks = list(flanks or [FLANK] * (len(gaps) + 1))
    assert len(flanks) == len(gaps) + 1 and min(flanks) >= k + 1
    rng = np.random.default_rng(seed)
    total = sum(flanks) + sum(g["true_len"] for g in gaps)
    t = ["ACGT"[i] for i in rng.integers(0, 4, total)]
    starts, pos = [], 0
    for g, fl in zip(gaps, flanks):
        pos += fl
        starts.append(pos)
        n, rep = g["true_len"], k + 20
        for a, b in g.get("repeats", ()):
            assert 0 < a and a + rep <= b and b + rep < n
            t[pos + b:pos + b + rep] = t[pos + a:pos + a + rep]
        for p in (pos, pos + n - 1):
            # the gap's first and last base differ from their neighbours: deleting one, or inserting beside it, is not the
            # same edit one place further, so the regions end exactly where the flanks do
            t[p] = next(c for c in "ACGT" if c != t[p - 1] and c != t[p + 1])
        pos += n
    t = "".join(t)
    R = GapRead()
    R.k, R.truth, R.transcripts, R.gaps, R.regions = k, t, [t], [], []
    pieces, reg_start, read_pos = [], 0, 0
    for gi, (g, s0) in enumerate(zip(gaps, starts)):
        comb, period, n, sites = g.get("comb", "sub"), g.get("period", 15), g["true_len"], tuple(g.get("sites", ()))
        assert comb in ("sub", "del", "ins") and period < k
        assert all(0 < s < n - 1 and s % period == 0 for s in sites) and all(b - a >= k for a, b in zip(sites, sites[1:]))
        alt = {}
        for s in sites:
            p = s0 + s
            alt[s] = _other(t[p], rng)
            R.transcripts.append(t[p - k + 1:p] + alt[s] + t[p + 1:p + k])
        decisive = tuple(g.get("decisive", ()))
        assert all(0 < s < n - 1 and s % period not in (0, 1, period - 1) for s in decisive)
        assert all(b - a >= k for a, b in zip(sorted(sites + decisive), sorted(sites + decisive)[1:]))
        for s in decisive:                              # (a generator of its own: the comb's teeth stay what they are without)
            p = s0 + s
            R.transcripts.append(t[p - k + 1:p] + _other(t[p], np.random.default_rng(seed * 100003 + s)) + t[p + 1:p + k])
        out, last = [], 0
        for m in sorted(set(list(range(0, n, period)) + [n - 1])):
            out.append(t[s0 + last:s0 + m])
            here, before, after = t[s0 + m], t[s0 + m - 1], t[s0 + m + 1]
            third = _other(here, rng, alt[m]) if m in alt else None
            if comb == "sub" or third:
                out.append(third or _other(here, rng))
            elif comb == "ins" and m == n - 1:
                # (after the gap's last base: neither that base nor the flank's first, so the read's gap ends here)
                out.append(here + [c for c in "ACGT" if c != here and c != after][int(rng.integers(0, 2))])
            elif comb == "ins":
                # a base that is neither neighbour's: the read's gap really is one base longer here
                out.append([c for c in "ACGT" if c != here and c != before][int(rng.integers(0, 2))] + here)
            last = m + 1
        out.append(t[s0 + last:s0 + n])
        rgap = "".join(out)
        pieces += [t[s0 - flanks[gi]:s0], rgap]
        G = Gap()
        G.comb, G.true_len, G.true_start, G.sites, G.repeats = comb, n, s0, sites, tuple(g.get("repeats", ()))
        G.decisive = decisive
        G.start = read_pos + flanks[gi]
        G.read_gap, G.flank_r = len(rgap), flanks[gi + 1]
        G.ref_len, G.path_max = ref_len(G.read_gap, G.flank_r, k), path_max(G.read_gap, k)
        R.regions.append((reg_start, G.start - k))
        reg_start = G.start + G.read_gap
        read_pos = reg_start
        R.gaps.append(G)
    pieces.append(t[len(t) - flanks[-1]:])
    R.read = "".join(pieces)
    R.regions.append((reg_start, len(R.read) - k))
    if len(gaps) == 1:
        for f, v in vars(R.gaps[0]).items():
            setattr(R, f, v)
    return R


def gap_read(true_len, k=K_DEFAULT, seed=1, flank_l=FLANK, flank_r=FLANK, **gap_kw):
    return multi_gap_read([dict(true_len=true_len, **gap_kw)], k=k, seed=seed, flanks=(flank_l, flank_r))


# ---------------------------------------------------------------- the oracle's trace
def runs(trace_text):
    """Per search of a trace and per start anchor: dict(location, direction, steps, sizes, full, found) — the `6` lines'
    step, Trails after the step and bridges recorded so far; found: the `5` line's flag."""
    out = []
    cur = None
    for line in trace_text.splitlines():
        f = line.split(" ")
        if f[0] == "3":
            cur = dict(location=int(f[1]), direction=int(f[2]), runs=[], found=None)
            out.append(cur)
        elif f[0] == "6" and cur is not None:
            if int(f[1]) == 1 or not cur["runs"]:
                cur["runs"].append(dict(steps=[], sizes=[], full=[]))
            r = cur["runs"][-1]
            r["steps"].append(int(f[1]))
            r["sizes"].append(int(f[2]))
            r["full"].append(int(f[3]))
        elif f[0] == "5" and cur is not None and cur["found"] is None:
            cur["found"] = int(f[2])
    return out


def size_changes(run):
    """[(step, Trails after it)] at the steps where the number of Trails changes."""
    s, n = run["steps"], run["sizes"]
    return [(s[i], n[i]) for i in range(len(s)) if i == 0 or n[i] != n[i - 1]]


def last_step_with(run, at_least):
    return max([s for s, n in zip(run["steps"], run["sizes"]) if n >= at_least], default=0)


def check_steps(run, interval, more_than):
    """The steps of a run after which its Trails were scored: check_interval divides the step and more Trails than
    max_nb_competing_paths came out of it.  (With the sites' ties gardening keeps them all, so the trace's size after the
    step is the size that was scored; a case whose sizes drop on a check step says so in its facts.)"""
    return [s for s, n in zip(run["steps"], run["sizes"]) if s % interval == 0 and n > more_than]


# ---------------------------------------------------------------- the cases
TWO = dict(max_nb_competing_paths=1)        # two Trails are "complex": scored on every check step
TOP = dict(max_nb_competing_paths=64, max_nb_inner_paths=60)


def _flank_for(ref, k):
    """A right flank short enough that the bridge's identity (LCS over refLen, which counts the whole target region)
    stays above min_inner_score = 0.7: a fifth of the reference, 400 at most."""
    return min(FLANK, max(2 * k, (ref - k) // 5))


def _two_trail_sub(ref, k=K_DEFAULT, seed=1, back=300, scorings=7):
    """Substitution comb with refLen == ref, one site `back` bases before the gap's end (half the gap at most), and the
    check_interval that scores the two Trails about `scorings` times before they outgrow the reference."""
    fr = _flank_for(ref, k)
    g = ref - fr - k
    site = (g - min(back, g // 2)) // 15 * 15
    alive = ref - k - site                                   # steps from the site to a Trail of more than refLen bases
    ci = max(2, alive // scorings)
    return (dict(true_len=g, k=k, seed=seed, flank_r=fr, sites=(site,), decisive=(_decisive_after(site, ci, k),)),
            dict(TWO, check_interval=ci))


def _decisive_after(site, ci, k, period=15):
    """The first offset between two teeth that is K or more beyond a tie site and leaves a check step between the two:
    the two Trails have been scored, and have rows kept, when they double again."""
    s = site + max(k, ci + 1)
    while s % period != period // 2:
        s += 1
    return s


def _lone(read_gap, k=K_DEFAULT, seed=1, **kw):
    return dict(true_len=read_gap, k=k, seed=seed, flank_r=_flank_for(read_gap + 200, k), **kw), {}


CASES = {}        # name -> (gap_read keywords or a list of gap dicts, parameter keywords, what it is there for)

# -- the reference length at ROW_MAX_REF: kept rows at 8190 and 8191, every Trail from scratch at 8192 (four scorings
#    there, not seven: from scratch each costs the HIP path 0.2 s per Trail and the oracle 0.25 s)
for _ref in (8190, 8191, 8192):
    _b, _p = _two_trail_sub(_ref, seed=20 + _ref % 10, scorings=7 if _ref <= ROW_MAX_REF else 4)
    CASES["ref-%d" % _ref] = (_b, _p, dict(ref=_ref, records=row_records(_ref), two_trails=True, boundary=True))

# -- the Trail passes 8191 bases while the reference does not (score_bridges drops the kept rows for that scoring), and
#    the mirror image: the reference is beyond 8191 and no Trail gets there (7600 + 400 + K = 8021).  Two Trails tie at
#    a substituted site of a deletion or insertion comb for some transcripts and not for others (the alignment may
#    move a tooth's gap next to the site): the seeds are ones for which they do, and the CPU file asserts it
#    The decisive site of trail-past-8191 lies before 8191: once a Trail is longer than the whole reference its newest
#    ~100 bases are outside what the alignment scores (its end is free), so nothing that enters a Trail after step ~8100
#    ever changes a score.  The site at 8017 is decided at step 8200, the first scoring that drops the kept rows
CASES["trail-past-8191"] = (dict(true_len=8250, comb="del", sites=(7950,), decisive=(8017,), seed=33), dict(TWO, check_interval=50),
                            dict(two_trails=True, boundary=True, trail_past=True))
CASES["ref-past-8191-trail-below"] = (dict(true_len=7600, comb="ins", period=20, sites=(7300,), decisive=(7450,), seed=31), dict(TWO, check_interval=570),
                                      dict(two_trails=True, boundary=True, trail_below=True))

# -- every score_bridges_rows<N>: the longest reference of each instance, and the first of the next for <2>, <4>, <6>
#    and <96> (8191 | 8192, the end of <128>, are above)
_INSTANCE_REFS = [64 * n for n in INSTANCES[:-1]] + [64 * n + 1 for n in (2, 4, 6, 96)]
for _ref in sorted(_INSTANCE_REFS):
    _b, _p = _two_trail_sub(_ref, seed=40 + _ref % 7)
    CASES["instance-%d-ref-%d" % (instance_of(_ref), _ref)] = (_b, _p, dict(ref=_ref, instance=instance_of(_ref), two_trails=True))

# -- 57 records for up to 64 Trails: six sites in the gap's last 180 bases under the 64 / 60 limits
_g = 8000 - FLANK - K_DEFAULT
_s = (_g - 180) // 15 * 15
CASES["row-arena"] = (dict(true_len=_g, sites=tuple(_s + 30 * i for i in range(6)), seed=51), dict(TOP, check_interval=6),
                      dict(ref=8000, records=57, trails=64))

# -- the cycle filter: pathMax at WIDE_BLOOM_MIN_PATH (the wide one is used above 600), then at every doubling of the wide
#    one (words < pathMax / 2); every second case with a repeat in its gap, ~100 bases on or most of the gap away
_b, _p = _lone(gap_with_path_max(WIDE_BLOOM_MIN_PATH, K_DEFAULT, False), seed=60, repeats=((200, 300),))
CASES["bloom-600"] = (_b, _p, dict(words=0, repeat=True))
_b, _p = _lone(gap_with_path_max(WIDE_BLOOM_MIN_PATH, K_DEFAULT, True), seed=61, repeats=((200, 300),))
CASES["bloom-601"] = (_b, _p, dict(words=1024, repeat=True))
for _i, _w in enumerate((1024, 2048, 4096, 8192, 16384)):
    _lo, _hi = gap_with_path_max(2 * _w + 1, K_DEFAULT, False), gap_with_path_max(2 * _w + 1, K_DEFAULT, True)
    _near, _far = ((300, 400),), ((300, _hi - 700),)
    # (at 27 kb a far repeat on either side: a bridge of 27 kb found costs the oracle 9 s, most of it the final alignment)
    _rep = _near if _i % 2 else ((300, _lo - 700),) if _w == WIDE_BLOOM_WORDS else ()
    _b, _p = _lone(_lo, seed=62 + 2 * _i, repeats=_rep)
    CASES["bloom-sizes-%d-below" % _w] = (_b, _p, dict(words=_w, repeat=bool(_rep)))
    _b, _p = _lone(_hi, seed=63 + 2 * _i, repeats=_far if _i % 2 == 0 else ())
    CASES["bloom-sizes-%d-above" % _w] = (_b, _p, dict(words=min(2 * _w, WIDE_BLOOM_WORDS), repeat=_i % 2 == 0))

# -- one read, three searches of one wave: two gaps with the same reference length, a third with another
CASES["two-long-gaps"] = ([dict(true_len=5000, sites=(4695,), decisive=(4897,)), dict(true_len=5000, sites=(4695,), decisive=(4897,)),
                           dict(true_len=3000, sites=(2700,), decisive=(2857,))],
                          dict(TWO, check_interval=200), dict(two_trails=True, refs=(5421, 5421, 3421)))

# -- a search that outgrows its share of the first pass's arena without a hook.  A 12 kb gap leaves 72 buffers of
#    14.5 KB in the 1 MiB arena, which hold the 64 Trails six sites make (a child takes over its parent's buffer); at
#    14 kb the stride is 16 912 bytes, 62 buffers, and the step that makes 64 Trails of 32 cannot be served
_g = 14000
_s = (_g - 180) // 15 * 15
CASES["retry-for-real"] = (dict(true_len=_g, sites=tuple(_s + 30 * i for i in range(6)), seed=71), dict(TOP, check_interval=6),
                           dict(trails=64, retry=True))

# -- a scoring with records for some Trails and none for others: param_limit_cases.ladder (sites of 4, 4, 3, 4, 4 alleles
#    24 bases apart, the read with the backbone's) deep inside a noisy stretch of 2296 bases.  refLen 2617 leaves 175 records;
#    the 48 Trails make 192 candidates on a check step, all scored at once — at least 17 of them in buffers at or above
#    rowAvail, aligned from scratch beside those that go on from kept rows — and gardening, by the scores, keeps four.
#    The twin (check_interval 5: no check on that step) shows the 192.
_LADDER = dict(ways=(4, 4, 3, 4, 4), gap=24, k=K_DEFAULT, seed=11, margin=1100, first_site=1400, length=2896)
CASES["row-arena-scored"] = (dict(ladder=_LADDER), dict(TOP, check_interval=1), dict(records=175, candidates=192, cut=True))
CASES["row-arena-scored-twin"] = (dict(ladder=_LADDER), dict(TOP, check_interval=5), dict(records=175, candidates=192))

BOUNDARY = [n for n, c in CASES.items() if c[2].get("boundary")]


def ladder_read(**kw):
    """A ladder of param_limit_cases as a GapRead: one gap, the noisy stretch."""
    import param_limit_cases as PL
    lad = PL.ladder(**kw)
    lo, hi = lad.noisy
    k, n = lad.k, len(lad.read)
    R, G = GapRead(), Gap()
    G.comb, G.true_len, G.true_start, G.start, G.sites, G.decisive, G.repeats = "ladder", hi - lo, lo, lo, (), (), ()
    G.ladder_sites = tuple(s - lo for s in lad.sites)
    G.read_gap, G.flank_r = hi - lo, n - hi
    G.ref_len, G.path_max = ref_len(G.read_gap, G.flank_r, k), path_max(G.read_gap, k)
    R.k, R.truth, R.transcripts, R.read, R.gaps = k, lad.backbone, lad.transcripts, lad.read, [G]
    R.regions = [(0, lo - k), (hi, n - k)]
    for f, v in vars(G).items():
        setattr(R, f, v)
    return R


def case(name):
    """(GapRead, parameter keywords, what it is there for)."""
    b, p, why = CASES[name]
    if isinstance(b, dict) and "ladder" in b:
        return ladder_read(**b["ladder"]), dict(p), dict(why)
    if isinstance(b, list):
        return multi_gap_read(b, seed=81), dict(p), dict(why)
    return gap_read(**b), dict(p), dict(why)


class OracleSide:
    """The oracle's half of a case, made once per process: g (GapRead), params, why, keys / counts (the table's dump),
    otab, trace (with step lines), status, out (the record), runs, seconds (CPU time of the trace on this thread) and
    score_calls (scoreBridges calls it took)."""


_oracle_side = {}


def packed_kmers(transcripts, k, depth=20):
    """(keys, counts) as parity_util.CustomPair stores a list of transcripts."""
    cnt = {}
    code = str.maketrans("ACGT", "0123")
    for t in transcripts:
        for i in range(len(t) - k + 1):
            cnt[t[i:i + k]] = cnt.get(t[i:i + k], 0) + depth
    keys = np.array([int(km.translate(code), 4) for km in cnt], dtype=np.uint64)
    return keys, np.fromiter(cnt.values(), dtype=np.uint32, count=len(cnt))


def oracle_table(transcripts, k, **pkw):
    import oracle_lib as O
    import parity_util as PU
    _, q = PU.both_params(k=k, **pkw)
    ot = O.OracleTable(q, O.OracleTable.FLAT)
    ot.insert_packed(*packed_kmers(transcripts, k))
    ot.decolour()
    return ot


def traced(otab, read):
    """(trace text with step lines, status, record, CPU seconds, scoreBridges calls) of one read."""
    import time
    import oracle_lib as O
    c0, t0 = O.ub_counters()["scoreBridgesCalls"], time.thread_time()
    text = otab.trace(read, steps=True)
    dt, calls = time.thread_time() - t0, O.ub_counters()["scoreBridgesCalls"] - c0
    lines = text.splitlines()
    status = next(int(l[7:]) for l in lines if l.startswith("STATUS "))
    return text, status, next(l[4:] for l in lines if l.startswith("OUT ")), dt, calls


def oracle_side(name):
    if name not in _oracle_side:
        s = OracleSide()
        s.name = name
        s.g, s.params, s.why = case(name)
        s.otab = oracle_table(s.g.transcripts, s.g.k, **s.params)
        s.trace, s.status, s.out, s.seconds, s.score_calls = traced(s.otab, s.g.read)
        s.runs = runs(s.trace)
        _oracle_side[name] = s
    return _oracle_side[name]


# ---------------------------------------------------------------- reads beyond 65 535 bases
def noisy(truth, rng, sub=0.04, dele=0.03, ins=0.03):
    """Per base of `truth` what the read has in its place: the base, another one, none, or the base and one more."""
    out = []
    draw = rng.random(len(truth))
    for b, r in zip(truth, draw):
        if r < sub:
            out.append(_other(b, rng))
        elif r < sub + dele:
            out.append("")
        elif r < sub + dele + ins:
            out.append(b + "ACGT"[int(rng.integers(0, 4))])
        else:
            out.append(b)
    return out


class LongReads:
    """transcripts, k, reads {name: text}, comb (the Gap-like facts of the comb read's gap: start, read_gap, ref_len,
    path_max)."""


LONG_COMB = 8300
LONG_N = 140_000


def long_reads(k=K_DEFAULT, seed=90):
    """Four reads from one random transcript: 65 535 + K and 65 537 + K bases with ~10 % mixed errors, one of 140 000
    bases with the same noise, and that read again with an 8.3 kb substitution comb between two clean stretches of 400
    bases in its middle."""
    rng = np.random.default_rng(seed)
    t = "".join("ACGT"[i] for i in rng.integers(0, 4, LONG_N + 3000))
    L = LongReads()
    L.k, L.transcripts, L.reads = k, [t], {}
    for name, n in (("65535+K", 65535 + k), ("65537+K", 65537 + k)):
        per = noisy(t, np.random.default_rng(seed + n % 100))
        text = "".join(per)
        # (cut to the length the case is named after: the 16-bit edge is the read's own length)
        L.reads[name] = text[:n]
        assert len(L.reads[name]) == n
    per = noisy(t, np.random.default_rng(seed + 7))
    ends = np.cumsum([len(x) for x in per])                  # ends[i]: read bases up to and with true base i
    cut = int(np.searchsorted(ends, LONG_N, side="right"))   # the true bases whose rendering fits 140 000 read bases
    L.reads["140k"] = "".join(per[:cut])
    a = 70_000
    b = a + FLANK + LONG_COMB + FLANK
    gap = [_other(c, rng) if (i % 15 == 0 or i == LONG_COMB - 1) else c for i, c in enumerate(t[a + FLANK:a + FLANK + LONG_COMB])]
    L.reads["140k-comb"] = "".join(per[:a]) + t[a:a + FLANK] + "".join(gap) + t[b - FLANK:b] + "".join(per[b:cut])
    G = Gap()
    G.start = int(ends[a - 1]) + FLANK
    G.read_gap, G.true_len, G.flank_r = LONG_COMB, LONG_COMB, None          # (the target region goes on into the noisy part)
    G.path_max = path_max(LONG_COMB, k)
    L.comb = G
    return L
