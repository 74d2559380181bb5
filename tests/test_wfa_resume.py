"""The carried wavefront of the unit-cost x-drop (talc_wfa.h: WfaKept / wfa_xdrop_scalar_run — the scalar statement of
what wave_xdrop_wfa keeps between the scorings of an edge's Trail, and of what the edge lane resumes from): run i + 1 of
the same pair, the query longer, x changed, resumed from the level run i kept, is the run a fresh start computes and the
extension the oracle's anti-diagonal x-drop reports."""
import ctypes as C
import random

import numpy as np

import oracle_lib as O
from talc_amd import build as B

ORC = O.lib()
ORC.orc_xdrop_right.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]


def pure():
    L = C.CDLL(B.build_pure())
    L.pure_wfa_xdrop.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    L.pure_wfa_xdrop_resume.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.pure_wfa_xdrop_resume.restype = C.c_int
    return L


P = pure()


def mutate(rnd, s, rate):
    out = []
    for ch in s:
        if rnd.random() < rate:
            op = rnd.random()
            if op < 0.6:
                out.append(rnd.choice([c for c in "ACGT" if c != ch]))
            elif op < 0.8:
                out.append(ch + rnd.choice("ACGT"))
        else:
            out.append(ch)
    return "".join(out)


def series(rnd, step, x_rule):
    """One pair: the query grows by `step` bases per run.  Yields (query, database, x, resumed, got, fresh, want)."""
    n = rnd.choice([40, 90, 160, 300])
    full = "".join(rnd.choice("ACGT") for _ in range(n))
    d = mutate(rnd, full, rnd.choice([0.0, 0.03, 0.08, 0.15, 0.25]))
    shape = rnd.choice(["shorter", "equal", "longer"])          # the database against the query at its full length
    if shape == "shorter":
        d = d[: max(1, len(d) - rnd.randint(1, n // 2))]
    elif shape == "longer":
        d = d + "".join(rnd.choice("ACGT") for _ in range(rnd.randint(1, 60)))
    else:
        d = (d + full)[:n]
    keep = np.zeros(130, dtype=np.int32)
    xd = int(step * 0.3 + 1.0)                                   # Explorer.cpp:1031 for a failure rate of 0.3
    qlen = 0
    while qlen < n:
        qlen = min(n, qlen + step)
        q = full[:qlen]
        if x_rule == "reference":
            x = xd + 2                                           # scoreEdges: the last x-drop plus 2 ...
        else:
            x = rnd.choice([0, 1, 2, 3, 5, 8, 12, 20, 31, 32, 45, rnd.randint(0, 70)])
        got, fresh, want = (np.zeros(4, dtype=np.int32) for _ in range(3))
        resumed = P.pure_wfa_xdrop_resume(q.encode(), len(q), d.encode(), len(d), x, keep.ctypes.data, got.ctypes.data)
        P.pure_wfa_xdrop(q.encode(), len(q), d.encode(), len(d), x, fresh.ctypes.data)
        ORC.orc_xdrop_right(q.encode(), d.encode(), 0, -1, -1, x, want.ctypes.data)
        yield q, d, x, resumed, got, fresh, want, shape
        if x_rule == "reference":
            if not got[0] or got[1] != qlen:                     # (the Trail fails its scoring: the search ends, mostly)
                if rnd.random() < 0.7:
                    return
            xd = -int(got[3])                                    # ... and minus the new score is the next one


def test_resumed_runs_equal_fresh_runs_and_the_oracle():
    rnd = random.Random(2024)
    runs = resumed_runs = 0
    by_rule = {"reference": [0, 0], "arbitrary": [0, 0]}
    shapes = set()
    for trial in range(1500):
        step = (1, 4, 6, 7, 13)[trial % 5]
        x_rule = "reference" if trial % 3 else "arbitrary"
        for q, d, x, resumed, got, fresh, want, shape in series(rnd, step, x_rule):
            assert (got == fresh).all(), (q, d, x, resumed, got.tolist(), fresh.tolist())
            assert want[0] == got[0], (q, d, x, resumed, want.tolist(), got.tolist())
            if want[0]:
                assert (want[1:] == got[1:]).all(), (q, d, x, resumed, want.tolist(), got.tolist())
            runs += 1
            resumed_runs += resumed
            by_rule[x_rule][0] += 1
            by_rule[x_rule][1] += resumed
            shapes.add(shape)
    print("runs %d, resumed %d; by rule %s" % (runs, resumed_runs, by_rule))
    assert shapes == {"shorter", "equal", "longer"}
    assert runs > 10000
    assert 2 * resumed_runs >= runs, (runs, resumed_runs)        # a test in which resumption never happens proves nothing
    assert by_rule["arbitrary"][1] > 500
