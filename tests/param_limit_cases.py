"""Inputs that take the path search to the upper ends of its parameter ranges (max_nb_competing_paths 64, max_nb_inner_paths
60, max_start_anchors 64, max_nb_border_paths and check_interval without an upper bound), and what the oracle's trace
says about them.  k_search runs one wavefront per read: a Trail set of more than 64 is a second or third pass of every
step loop, MAXB = 64 a full ballot, 64 anchors a full aim list.  Nothing here needs the product or a GPU:
tests/test_param_limits_reference.py asserts the reach of every case from the oracle alone, tests/test_gpu_param_limits.py
runs them through the HIP path.

The synthetic rows are stress_cases.CASES 406-416 (set 301's generator, whose paralogs fork most).  A ladder is a
hand-made graph: a random backbone with variant sites every `gap` bases, every allele stored with the same count, so that
a search walking it multiplies its Trail set by the site's number of alleles — 4 x 4 x 3 = 48 <= 60 Trails, then 192."""
import numpy as np

from stress_cases import CASES

HEAD, INNER, TAIL = 0, 1, 2           # the location of a search in the trace's `3` line (Explorer.h: Location)
WAVE = 64

# stress_cases number -> (what the row is there for, the reach conditions it claims, how many of the generator's first reads
# it takes).  "sets": at least 100 of 200 reads have a Trail set above 64, and head, inner and tail searches each have one;
# "garden": gardening is called on more than MAXB = 64 candidates (cuts_against_twin); "anchors": a search lists 64 or more
# anchors on a side.  The rows that claim nothing are the other parameters' ends and other K over the same generator.
# 200 reads, but for the rows whose 200 reads take the oracle (16 threads) 8.7 s (check_interval = 1 scores every Trail on
# every step), 6.5 s (a border limit of 0 or 1 scores every step of every edge) and 15 s (K = 31: reads to 20 kb): those
# take as many as it corrects in a few seconds.  None of them claims "sets", whose bound is stated for 200 reads.
SYNTHETIC = {
    406: ("MAXB64-INNER60", ("sets",), 200),
    407: ("MAXB63-INNER59", ("sets",), 200),
    408: ("MAXB64-INNER60-CI1", ("garden",), 100),
    409: ("MAXB64-INNER60-CI40-BORDER300", ("sets",), 200),
    410: ("MAXB64-INNER60-ANCHORS64-64", ("sets", "anchors"), 200),
    411: ("MAXB64-INNER60-ANCHORS1-MIN63", ("sets", "anchors"), 200),
    412: ("BORDER1", (), 100),
    413: ("MAXB64-INNER60-k31-mixed", (), 60),
    414: ("MAXB64-INNER60-k18", ("sets",), 200),
    415: ("MAXB64-INNER60-reverse", ("sets",), 200),
    416: ("BORDER0", (), 100),
}
GARDEN_TWIN = {408: 406}     # the same reads and parameters but for check_interval


def synthetic_row(case):
    """(Pair keywords, parameter keywords, number of reads) of a synthetic row."""
    kw, pkw = CASES[case]
    return dict(kw), dict(pkw), SYNTHETIC[case][2]


def row_reads(synth, case):
    """The reads of a row as texts: the generator's first ones, reverse complemented for a row with reverse = 1 (such a
    context works on the reverse complement of what it is given, main.cpp:253)."""
    import parity_util as PU
    seqs = PU.seqs_of(*synth.reads(0, SYNTHETIC[case][2]))
    return [PU.revcomp(s) for s in seqs] if CASES[case][1].get("reverse") else seqs


# ---------------------------------------------------------------- the oracle's trace
def searches(trace_text):
    """The searches of a trace in order: dicts of location, direction, nL / nR (anchors on either side: the `3` line),
    sizes (the Trail set after every step: the `6` lines, one list per start anchor — the step counter restarts at 1) and
    found (the `5` line's flag, None if the trace has none for the search)."""
    out = []
    for line in trace_text.splitlines():
        f = line.split(" ")
        if f[0] == "3":
            out.append(dict(location=int(f[1]), direction=int(f[2]), nL=int(f[3]), nR=int(f[4]), sizes=[], steps=[], found=None))
        elif f[0] == "6" and out:
            s = out[-1]
            if int(f[1]) == 1 or not s["sizes"]:
                s["sizes"].append([])
                s["steps"].append([])
            s["sizes"][-1].append(int(f[2]))
            s["steps"][-1].append(int(f[1]))
        elif f[0] == "5" and out and out[-1]["found"] is None:
            out[-1]["found"] = int(f[2])
    return out


def set_sizes(trace_text):
    """{location: [sizes after every step, over all searches and start anchors at that location]}."""
    per = {HEAD: [], INNER: [], TAIL: []}
    for s in searches(trace_text):
        for run in s["sizes"]:
            per[s["location"]].extend(run)
    return per


def largest_sets(trace_text):
    return {loc: max(v, default=0) for loc, v in set_sizes(trace_text).items()}


def _runs(trace_text):
    """Every start anchor's run of every search, in order: (location, direction, steps, sizes)."""
    return [(s["location"], s["direction"], steps, run) for s in searches(trace_text) for run, steps in zip(s["sizes"], s["steps"])]


def cuts_against_twin(trace_text, twin_text, maxb=WAVE):
    """Where a trace and its twin's (same read, same table, parameters that differ only in when a check happens) part:
    runs of the same search whose sets agree on every step before step s, where the twin shows `before` > maxb Trails
    and the trace fewer.  Up to there both made the same Trails, so on step s the trace's search made `before`
    candidates too and cut them: (location, direction, step, before, after, the trace's run goes on after it)."""
    out = []
    for (loc, d, steps, run), (loc2, d2, steps2, run2) in zip(_runs(trace_text), _runs(twin_text)):
        if (loc, d) != (loc2, d2):
            break
        n = min(len(run), len(run2))
        i = next((i for i in range(n) if run[i] != run2[i]), None)
        if i is None:
            if len(run) != len(run2):
                break                       # (the runs part without a differing step: nothing to say, and no common ground after)
            continue
        if steps[i] == steps2[i] and run2[i] > maxb and run[i] < run2[i]:
            out.append((loc, d, steps[i], run2[i], run[i], len(run) > i + 1))
        break                               # after the first difference the two searches are no longer the same
    return out


def max_anchors(trace_text):
    return max([max(s["nL"], s["nR"]) for s in searches(trace_text)], default=0)


# ---------------------------------------------------------------- ladders
class Ladder:
    """What ladder() returns: transcripts (for parity_util.CustomPair), read (the noisy read), backbone, sites (their
    positions in the backbone), alleles (per site, the backbone's base first), k, form."""


def _other_bases(b, n, rng):
    rest = [c for c in "ACGT" if c != b]
    rng.shuffle(rest)
    return rest[:n]


def ladder(ways, gap, k, seed, form="bridge", length=1400, first_site=400, noise=0.12, margin=40, clean=300):
    """A backbone of `length` random bases with a variant site every `gap` bases (gap > k: a k-mer spans at most one
    site) from `first_site`, ways[i] alleles at site i.  The transcripts are the backbone plus, for every alternative
    allele, the 2 k - 1 bases around its site: every k-mer that holds the allele, once, so every stored k-mer has the same
    count.  The read is the backbone with `noise` substitutions from `margin` bases before the first site to `margin`
    after the last — solid on both sides of the ladder, which a *bridge* search then walks from the left anchor.
    form "tail": the backbone ends `margin` bases after the last site (transcripts and read), so nothing solid lies
    beyond the ladder and the *edge* search of the read's tail walks it; the read's last `clean` bases before the noisy
    stretch are kept clean by moving the sites, not by the form.  form "head": the mirror image, by reverse complement
    of the tail form — the head search walks LEFT through the ladder."""
    assert gap > k and all(2 <= w <= 4 for w in ways) and form in ("bridge", "head", "tail")
    rng = np.random.default_rng(seed)
    backbone = "".join("ACGT"[i] for i in rng.integers(0, 4, length))
    sites = [first_site + i * gap for i in range(len(ways))]
    lo, hi = sites[0] - margin, sites[-1] + margin
    assert clean <= lo and hi + clean <= length
    if form != "bridge":
        backbone = backbone[:hi]
    alleles = [[backbone[s]] + _other_bases(backbone[s], w - 1, rng) for s, w in zip(sites, ways)]
    transcripts = [backbone]
    for s, al in zip(sites, alleles):
        for b in al[1:]:
            transcripts.append(backbone[s - k + 1:s] + b + backbone[s + 1:s + k])
    read = list(backbone)
    site_set = set(sites)
    last = lo - 1
    for i in range(lo, hi):
        # a site keeps the backbone's allele in the read (a substitution there could land on another allele).  The first
        # and the last base of the stretch are substituted and no k - 2 bases in a row are left clean, so the stretch
        # holds no solid k-mer, the anchors are the k-mers that end at lo - 1 and start at hi, and the search that starts
        # there adds the base of site i on its step (site - lo + 1): which steps fork is known from the arguments
        if i not in site_set and (i in (lo, hi - 1) or i - last >= k - 2 or rng.random() < noise):
            read[i] = _other_bases(backbone[i], 1, rng)[0]
            last = i
    L = Ladder()
    L.k, L.form, L.ways, L.gap, L.sites, L.alleles = k, form, list(ways), gap, sites, alleles
    L.backbone, L.transcripts, L.read, L.noisy = backbone, transcripts, "".join(read), (lo, hi)
    if form == "head":
        import parity_util as PU
        L.backbone, L.read = PU.revcomp(L.backbone), PU.revcomp(L.read)
        L.transcripts = [PU.revcomp(t) for t in transcripts]
        n = len(L.backbone)
        L.sites = [n - 1 - s for s in reversed(sites)]
        L.alleles = [[b.translate(PU.COMP) for b in al] for al in reversed(alleles)]
        L.ways = list(reversed(L.ways))
        L.noisy = (n - hi, n - lo)
    return L


def kmer_counts(transcripts, k):
    """{k-mer text: occurrences over the transcripts} — what CustomPair stores, before its `depth`."""
    cnt = {}
    for t in transcripts:
        for i in range(len(t) - k + 1):
            cnt[t[i:i + k]] = cnt.get(t[i:i + k], 0) + 1
    return cnt


def sites_spanned(lad):
    """Per stored k-mer, how many sites it spans: every k-mer is a window of the backbone but for the alleles, so its
    place is found by matching it against the backbone with the sites left out."""
    k, bb = lad.k, lad.backbone
    site_set = set(lad.sites)
    where = {}
    for i in range(len(bb) - k + 1):
        key = "".join("." if j in site_set else bb[j] for j in range(i, i + k))
        where.setdefault(key, []).append(i)
    out = {}
    for km in kmer_counts(lad.transcripts, k):
        hits = []
        for key, pos in where.items():
            if all(a == "." or a == b for a, b in zip(key, km)):
                hits += pos
        assert len(hits) == 1, (km, hits)
        out[km] = sum(1 for j in range(hits[0], hits[0] + k) if j in site_set)
    return out


# name -> (ladder keywords, parameter keywords, what it is there for).  A search from the left anchor adds site i on step
# margin + 1 + i * gap, one from the right anchor on step margin + (sites - 1 - i) * gap; a bridge search cuts its set only
# on a step that check_interval divides and only above MAXB Trails, an edge search on such a step or at
# max_nb_border_paths Trails.  "visible": the set named is what the trace shows after the step (no check on it), and the
# search ends there, above max_nb_inner_paths.  "cut": the same set is made on a check step, gardening (after scoreEdges in
# an edge search) gets all of it, and the search goes on with what is kept — seen against the "visible" twin of the same
# ladder, whose trace is the same up to that step.  "scored": an edge search reaches max_nb_border_paths on that step, so
# scoreEdges extends all of the set and gardening ranks it with MAXB = 64; the alleles of the last site lie beyond what is
# aligned, every Trail ties, all are kept.
_TOP = dict(max_nb_competing_paths=64, max_nb_inner_paths=60)
_EDGE = dict(_TOP, check_interval=50, max_nb_border_paths=300)
_L5 = dict(ways=(4, 4, 3, 4, 4), gap=24, k=21, seed=11)          # 4 x 4 x 3 = 48, then 192 on step 113 (from the right: 112)
_L3 = dict(ways=(3, 3, 3, 3, 3), gap=24, k=21, seed=13)          # 27, then 81 on step 113 (112)
LADDERS = {
    "bridge-k21-44344-ci5": (_L5, dict(_TOP, check_interval=5), dict(visible=192, location=INNER)),
    "bridge-k21-44344-maxb48-ci3": (_L5, dict(_TOP, max_nb_competing_paths=48, check_interval=3), dict(visible=192, location=INNER)),
    "bridge-k21-44344-ci1": (_L5, dict(_TOP, check_interval=1), dict(cut=192, twin="bridge-k21-44344-ci5", location=INNER)),
    "bridge-k21-44344-ci2": (_L5, dict(_TOP, check_interval=2), dict(cut=192, twin="bridge-k21-44344-ci5", location=INNER)),   # (112: from the right)
    "bridge-k21-33333-ci5": (_L3, dict(_TOP, check_interval=5), dict(visible=81, location=INNER)),
    "bridge-k21-33333-ci1": (_L3, dict(_TOP, check_interval=1), dict(cut=81, twin="bridge-k21-33333-ci5", location=INNER)),
    "bridge-k18-2344-ci6": (dict(ways=(2, 3, 4, 4), gap=20, k=18, seed=14), dict(_TOP, check_interval=6), dict(visible=96, location=INNER)),
    "bridge-k31-44344-ci6": (dict(ways=(4, 4, 3, 4, 4), gap=35, k=31, seed=15), dict(_TOP, check_interval=6), dict(visible=192, location=INNER)),
    "tail-k21-44344": (dict(_L5, seed=16, form="tail"), _EDGE, dict(visible=192, location=TAIL)),
    "tail-k21-44344-border100": (dict(_L5, seed=16, form="tail"), dict(_EDGE, max_nb_border_paths=100), dict(scored=192, twin="tail-k21-44344", location=TAIL)),
    "head-k21-44344": (dict(_L5, seed=17, form="head"), _EDGE, dict(visible=192, location=HEAD)),
    "head-k21-44344-border100": (dict(_L5, seed=17, form="head"), dict(_EDGE, max_nb_border_paths=100), dict(scored=192, twin="head-k21-44344", location=HEAD)),
    "tail-k31-3333": (dict(ways=(3, 3, 3, 3), gap=33, k=31, seed=18, form="tail"), _EDGE, dict(visible=81, location=TAIL)),
    "head-k18-2344": (dict(ways=(2, 3, 4, 4), gap=19, k=18, seed=19, form="head"), _EDGE, dict(visible=96, location=HEAD)),
}


def ladder_case(name):
    """(Ladder, parameter keywords, what it is there for)."""
    lkw, pkw, why = LADDERS[name]
    return ladder(**lkw), dict(pkw), dict(why)


# ---------------------------------------------------------------- the bush: more survivors than a Trail set was sized for
class Bush:
    """What bush() returns: keys / counts (the k-mers, packed as the tables take them), read, backbone, leaves, k."""


def bush(k=21, seed=31, length=1400, first_site=400, margin=40, depth=20, fans=((4,), (4,) * 4, (4,) * 11 + (3,) * 5)):
    """A graph on which gardening's "complex" branch (Explorer.cpp:852 ff.) keeps MAXB + n - 4 of n = 240 candidates: 300
    with MAXB = 64.  Five sites 5 bases apart (so the k-mer that ends on the last one still holds the first: which alleles
    may follow depends on all alleles before, and the paths through the graph are exactly the haplotypes stored).  Sites
    0-2 fork as `fans` says (4, 16, then 59 Trails); at site 3 one Trail alone forks in two (60 Trails, the most a search
    goes on with), the read agrees with the other 59 there and has N at the other four sites; at site 4 every Trail forks
    four ways.  All k-mers have one count but the 236 last ones of the 59: a count one higher, so a distance above that of
    the four children of the Trail that took the other base at site 3 — which score lower.  No candidate is first by
    score and by distance, 236 tie for the best score, and the reference keeps the 64 nearest of them and then all 236."""
    rng = np.random.default_rng(seed)
    backbone = "".join("ACGT"[i] for i in rng.integers(0, 4, length))
    sites = [first_site + 5 * j for j in range(5)]
    assert sites[-1] - sites[0] == k - 1 or k != 21
    assert sites[-1] - sites[0] <= k - 1
    lo, hi = sites[0] - margin, sites[-1] + margin

    def others(pos, n):
        return [backbone[pos]] + [c for c in "ACGT" if c != backbone[pos]][:n - 1]

    level = [()]
    for j, fan in enumerate(fans):                      # sites 0, 1, 2: node i of the level has fan[i] children
        assert len(fan) == len(level)
        level = [h + (b,) for h, f in zip(level, fan) for b in others(sites[j], f)]
    assert len(level) == 59
    odd = level[-1] + (others(sites[3], 2)[1],)         # site 3: the backbone's base for all, and one Trail with another too
    level = [h + (backbone[sites[3]],) for h in level] + [odd]
    leaves = [h + (b,) for h in level for b in others(sites[4], 4)]
    assert len(level) == 60 and len(leaves) == 240
    cnt = {}
    code = str.maketrans("ACGT", "0123")
    for i in range(length - k + 1):
        cnt[backbone[i:i + k]] = depth
    for h in leaves:
        t = list(backbone)
        for s, b in zip(sites, h):
            t[s] = b
        t = "".join(t)
        for e in range(sites[0], sites[4] + 1):         # the k-mers that end between the first site and the last
            km = t[e - k + 1:e + 1]
            last = e == sites[4] and h[3] == backbone[sites[3]]
            cnt[km] = depth + 1 if last else cnt.get(km, depth)
    read = list(backbone)
    last = lo - 1
    for i in range(lo, hi):
        if i in sites:
            if i != sites[3]:
                read[i] = "N"
            last = i
        elif i in (lo, hi - 1) or (i - last >= k - 2) or (rng.random() < 0.12 and not sites[0] - 3 <= i <= sites[4] + 3):
            read[i] = [c for c in "ACGT" if c != backbone[i]][int(rng.integers(0, 3))]
            last = i
    B = Bush()
    B.k, B.backbone, B.read, B.leaves, B.sites = k, backbone, "".join(read), leaves, sites
    B.keys = np.array([int(km.translate(code), 4) for km in cnt], dtype=np.uint64)
    B.counts = np.array(list(cnt.values()), dtype=np.uint32)
    return B


BUSH_PARAMS = dict(max_nb_competing_paths=64, max_nb_inner_paths=60, check_interval=1)
