"""Edge cases of the stakeholder-reasons scoring (jsim_score_trajectories) as data: situations chosen for the
kernel's structure -- four sequential passes that work in 64-element chunks and carry a running value from one chunk to the next, a
320-sample table, a 65536-step bound, a 512-thread stride over the weight rows -- not for the reference's behaviour.  No RNG: every
candidate is a straight or gently bent line whose raw spacing (0.00137, 0.00371, 0.0171 m ...) keeps arc length / step clear of the
integers, cut at the raw point that gives the wanted sample count or Euler step count; every target and every margin is asserted
when the cases are built (a case that breaks one is replaced here, never left out by a test).

cases() is what tests/golden/make_golden_reasons_edges.py turns into tests/golden/reasons_edges.npz and what the CPU and GPU tests
share; restated() is the numpy restatement (tests/reasons_numpy.py) on every case, computed once."""
import functools
import hashlib
import os

import numpy as np

import reasons_numpy as RN
from conftest import GOLDEN

N = np.pi / 2
VMAX = float(RN.DEFAULT_PAR[2])
FIXED_ROW = (1 / 9, 4 / 9, 4 / 9)
W_FIXED = (0.2, 0.5, 0.3)
# the weight rows of the main launch (policymaker, driver, cyclist; form): the reference's two, both clamps of form 1 and the same rows
# unclamped, the all-zero row in both forms, and four rows that lean on one stakeholder each
ROWS = [(FIXED_ROW, 0), (W_FIXED, 1), ((0.4, 0.4, 0.4), 1), ((3.0, 3.0, 3.0), 1), ((0.4, 0.4, 0.4), 0), ((3.0, 3.0, 3.0), 0),
        ((0.0, 0.0, 0.0), 1), ((0.0, 0.0, 0.0), 0), ((0.7, 0.2, 0.1), 1), ((0.1, 0.2, 0.7), 0), ((0.1, 0.1, 0.8), 1), ((0.8, 0.1, 0.1), 0)]
ROWS_W, ROWS_F = [r[0] for r in ROWS], [r[1] for r in ROWS]
OTHER_IDEAL = (0.5, 0.3, 0.2)                                        # (cyclist, driver, policymaker)
SWEEP_W = (1, 511, 512, 513, 1025)                                   # stage two strides by the 512-thread workgroup
REF_MAX_NB = 4000                                                    # the reference's Python loops stay cheap below this
MARGIN = {"floor": 1e-6, "ct": 1e-9, "range": 1e-9, "timer": 1e-9, "top": 1e-9}


def par(**over):
    p = RN.DEFAULT_PAR.copy()
    for k, v in over.items():
        p[RN.PAR_NAMES.index(k)] = v
    return p


def line(n, spacing, x=2.0, y0=-20.0, bend=0.0):
    """n raw points going up the road from (x, y0); bend > 0 drifts left by bend * s * s."""
    s = np.arange(n) * spacing
    return np.stack([x - bend * s * s, y0 + s, np.full(n, N)], 1)


def floor_ratio(pts, mode, v, p):
    """cum / dl per raw point, as the restatement's resample_curve forms it."""
    pts = np.asarray(pts, dtype=np.float64)
    d = pts[1:, :2] - pts[:-1, :2]
    cum = np.cumsum(np.append(0.0, np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])))
    return cum / RN.resample_step(len(pts), mode, v, p)


def cut_m(full, mode, v, p, m):
    """The shortest prefix of `full` that resamples to m points with its last point kept only because it is the last."""
    k = np.floor(floor_ratio(full, mode, v, p))                       # prefix-invariant: cum and dl of a prefix are the full line's
    step = np.append(True, (k[1:] - k[:-1]) >= 1.0)
    kept = np.cumsum(step)
    count = kept + np.where(step, 0, 1)                               # m of the prefix that ends at each point
    hit = np.nonzero((count == m) & ~step)[0]
    assert len(hit), (m, int(count[-1]))
    return full[:int(hit[0]) + 1]


def cut_nb(full, mode, v, p, nb):
    """The prefix of `full` whose completion time is nearest the middle of Euler step count nb (ct / DT = nb - 0.5)."""
    def ratio(n):
        st, R = RN.resample_candidate(full[:n], mode, (0.0, 0.0, 0.0, v), p)
        return RN.completion_time(R, v, p) / p[0] if st == 0 else 0.0
    lo, hi = 3, len(full)
    assert ratio(hi) >= nb - 0.5, (nb, ratio(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ratio(mid) >= nb - 0.5 else (mid, hi)
    assert nb - 0.9 < ratio(hi) < nb - 0.1, (nb, ratio(hi))
    return full[:hi]


def case(label, cands, v, cyc, now=(0.9, 0.8, 1.0, 7.55, 4.05), p=None, modes=None, time_from=None, want=None):
    """want: what the case was built for, {candidate index: {"m" | "nb" | "status" | "n": value}}, asserted in cases()."""
    c = {"label": label, "candidates": [np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3) for t in cands], "ego": (2.0, -20.0, N, float(v)),
         "cyclist": tuple(float(x) for x in cyc), "now": tuple(float(x) for x in now), "par": RN.DEFAULT_PAR.copy() if p is None else p,
         "default_par": p is None, "want": want or {}}
    if modes is not None:
        c["modes"], c["time_from"] = list(modes), list(time_from)
    return c


def layout(c):
    if "modes" in c:
        return c["modes"], c["time_from"]
    return RN.default_layout(len(c["candidates"]))


def situation(c):
    return {k: c[k] for k in ("candidates", "ego", "cyclist", "now", "par", "modes", "time_from") if k in c}


def restate(c, weights=ROWS_W, forms=ROWS_F, ideal=RN.IDEAL):
    modes, tf = layout(c)
    return RN.score_situation(c["candidates"], modes, tf, c["ego"], c["cyclist"], c["now"], c["par"], weights, forms, ideal)


def timers(r, now, p):
    """The two timers after each sample (NaN where the sample is out of range), accumulated in order as score_samples does."""
    out = np.full((2, r["n_samples"]), np.nan)
    for q, (flags, t) in enumerate(((r["in_d"], now[3]), (r["in_c"], now[4]))):
        for j in range(r["n_samples"]):
            if flags[j]:
                t += p[0]
                out[q, j] = t
    return out


def first_cross(r, now, p):
    """Per timer the index of the first sample at which it is at or past its threshold (-1: none)."""
    t = timers(r, now, p)
    hit = [np.nonzero(t[q] >= thr)[0] for q, thr in ((0, p[7]), (1, p[10]))]
    return tuple(int(h[0]) if len(h) else -1 for h in hit)


def now_for(c, cand, j_d, j_c):
    """The situation's two accumulators for which candidate `cand`'s timers first reach their thresholds at samples j_d and j_c,
    half a DT past them."""
    r = restate(c, [FIXED_ROW], [0])[0][cand]
    p, out = c["par"], list(c["now"])
    for q, (flags, j, thr) in enumerate(((r["in_d"], j_d, p[7]), (r["in_c"], j_c, p[10]))):
        assert flags[j], (c["label"], q, j)
        out[3 + q] = thr - (int(np.sum(flags[:j + 1])) - 0.5) * p[0]
        assert out[3 + q] >= 0.0, (c["label"], out)
    return dict(c, now=tuple(out))


def margins(c, res, scores):
    """The smallest distance of every discontinuous decision of one case from its boundary."""
    modes, _ = layout(c)
    p, v = c["par"], c["ego"][3]
    m = {k: np.inf for k in MARGIN}
    for pts, md, r in zip(c["candidates"], modes, res):
        if len(pts) >= 2 and not (md == 1 and not v > 0.0) and np.all(np.asarray(RN.resample_step(len(pts), md, v, p)) > 0.0):
            q = floor_ratio(pts, md, v, p)[1:]
            m["floor"] = min(m["floor"], float(np.min(np.abs(q - np.round(q)))))
        if np.isfinite(r["ct"]):
            q = r["ct"] / p[0]
            m["ct"] = min(m["ct"], abs(q - np.round(q)))
        if r["status"] == 0:
            m["range"] = min(m["range"], float(np.abs(r["dist"] - (p[5] + p[6])).min()), float(np.abs(r["dist"] - (p[8] + p[9])).min()))
            t = timers(r, c["now"], p)
            for q, thr in ((0, p[7]), (1, p[10])):
                if np.any(np.isfinite(t[q])):
                    m["timer"] = min(m["timer"], float(np.nanmin(np.abs(t[q] - thr))))
    for row in np.asarray(scores).reshape(len(scores), -1):
        s = np.sort(row[~np.isnan(row)])
        if len(s) > 1 and s[-1] != s[-2]:                             # a tie is exact; anything else is clear
            m["top"] = min(m["top"], float(s[-1] - s[-2]))
    return m


def _cyclist(k=0, straight=False):
    """A cyclist ahead and to the left of the ego; gently accelerating and steering unless the case has more than 200 Euler rows."""
    return (3.5, -17.0 + 0.9 * k, 1.4, N, 0.0, 0.0) if straight else (3.5, -17.0 + 0.9 * k, 1.4, N + 0.02, 0.1, -0.01)


def _build():
    out = []
    fine = line(2400, 0.00137)                                        # 3.3 m: the following candidate at 0.23 m/s, 23 mm a step
    mid = line(5200, 0.00371)                                         # 19.3 m: at 0.57 m/s, 57 mm a step
    road = line(8200, 0.0171)                                         # 140 m of road for the planned candidates
    # ---- sample count m on and next to every chunk edge and at the table's end; the following candidate (mode 1) is the subject,
    # the planned one before it gives the completion time
    for k, m in enumerate((3, 4, 63, 64, 65, 127, 128, 129)):
        donor = cut_nb(road, 0, 0.23, RN.DEFAULT_PAR, 9 + 2 * k)
        out.append(case(f"m = {m} (mode 1, v 0.23)", [donor, cut_m(fine, 1, 0.23, RN.DEFAULT_PAR, m)], 0.23, _cyclist(k), want={1: {"m": m}}))
    for k, m in enumerate((191, 192, 193, 255, 256, 320, 321)):
        donor = cut_nb(road, 0, 0.57, RN.DEFAULT_PAR, 12 + 3 * k)
        out.append(case(f"m = {m} (mode 1, v 0.57)", [donor, cut_m(mid, 1, 0.57, RN.DEFAULT_PAR, m)], 0.57, _cyclist(k),
                        want={1: {"m": m, "status": 4 if m > RN.MAX_RES else 0}}))
    far = line(7400, 0.0371)                                          # 274 m
    out.append(case("m = 319 (mode 0 below MAX_SPEED)", [cut_m(far, 0, 1.0, RN.DEFAULT_PAR, 319), mid[:300]], 1.0, _cyclist(0, True),
                    want={0: {"m": 319}}))
    slow = par(max_accel=0.00053)                                     # the per-point step and the per-segment speed grow all the way
    out.append(case("m = 257 (mode 0, MAX_ACCEL 0.00053: step and speed never saturate)", [cut_m(far, 0, 1.0, slow, 257), cut_m(mid, 1, 1.0, slow, 70)],
                    1.0, _cyclist(1, True), p=slow, want={0: {"m": 257}, 1: {"m": 70}}))
    ramp = par(max_accel=0.004, max_speed=6.0)                        # saturates in the twentieth raw chunk / third sample chunk
    out.append(case("m = 130 (mode 0, MAX_ACCEL 0.004: step saturates at raw point 1250)", [cut_m(line(6000, 0.0137), 0, 1.0, ramp, 130), mid[:250]],
                    1.0, _cyclist(2, True), p=ramp, want={0: {"m": 130}}))
    # ---- raw count n: the last raw chunk with 64, 1 and 2 valid lanes, the forced keep of the last point on lane 0
    ok = road[:1500]
    follow = line(30, 0.3137)
    def forced(n):                                                    # a spacing at which the last of n points is kept only because it is the last
        for sp in (0.3137, 0.3371, 0.2917, 0.3713):
            k = np.floor(floor_ratio(line(n, sp), 0, VMAX, RN.DEFAULT_PAR))
            if k[-1] == k[-2]:
                return sp
        raise AssertionError(n)
    for n, sp in ((2, 0.91), (3, 0.91), (64, 0.3137), (65, forced(65)), (128, 0.3137), (129, forced(129)), (64, 0.91), (65, 0.91)):
        cands, idx = ([line(n, sp), ok, follow], 0) if n == 2 else ([line(n, sp), follow], 0)
        out.append(case(f"n = {n} at {sp} m", cands, VMAX, _cyclist(n % 5), want={idx: {"n": n, "status": 2 if n == 2 else 0}}))
    # ---- Euler rows nb - 1 on and next to every chunk edge
    for k, nb in enumerate((2, 3, 64, 65, 66, 128, 129, 130)):
        out.append(case(f"nb - 1 = {nb - 1}", [cut_nb(road, 0, VMAX, RN.DEFAULT_PAR, nb), road[:400 + 37 * k]], VMAX, _cyclist(k),
                        want={0: {"nb": nb}, 1: {"nb": nb}}))
    out.append(case("many samples per Euler row: m = 129 over nb - 1 = 7", [cut_nb(road, 0, 0.23, RN.DEFAULT_PAR, 8), cut_m(fine, 1, 0.23, RN.DEFAULT_PAR, 129)],
                    0.23, (3.5, -19.0, 3.0, N + 0.05, 0.5, -0.02), want={1: {"m": 129, "nb": 8}}))
    out.append(case("Euler rows chunks apart: nb - 1 > 64 m at m = 4", [cut_nb(line(1500, 0.171), 0, 0.23, RN.DEFAULT_PAR, 284), cut_m(fine, 1, 0.23, RN.DEFAULT_PAR, 4)],
                    0.23, (3.5, -19.0, 1.4, N, 0.0, 0.0), want={1: {"m": 4, "nb": 284}}))
    for nb in (65536, 65537):                                         # five raw points kilometres apart: m = n, ct / DT = nb - 0.5
        leg = (nb - 0.5) * (RN.DEFAULT_PAR[0] * VMAX) / 4
        out.append(case(f"nb = {nb}", [line(5, leg)], VMAX, (3.5, -17.0, 1.4, N, 0.0, 0.0), modes=[0], time_from=[0],
                        want={0: {"m": 5, "nb": nb, "status": 0 if nb <= RN.MAX_STEPS else 4}}))
    # ---- timers: a cyclist standing beside the road puts a window of samples in range; the accumulators are then solved for the
    # sample at which each timer first reaches its threshold
    walk = line(3300, 0.01371)                                        # 45 m: the following candidate at 2 m/s, 0.2 m a step
    donor = cut_nb(road, 0, 2.0, RN.DEFAULT_PAR, 25)
    foll = cut_m(walk, 1, 2.0, RN.DEFAULT_PAR, 221)
    for centre, j_d, j_c in ((80, 63, 64), (80, 64, 63), (150, 128, 128)):
        c = case(f"timers first at their thresholds at samples {j_d} (driver) and {j_c} (cyclist)", [donor, foll], 2.0,
                 (5.0, -20.0 + 0.2 * centre + 0.037, 0.0, N, 0.0, 0.0), want={1: {"m": 221, "cross": (j_d, j_c)}})
        out.append(now_for(c, 1, j_d, j_c))
    for y in np.arange(-4.5, -3.5, 0.003):                            # the cyclist's window ends on lane 0 of the third chunk
        c = case("one sample of a chunk in range; driver timer past its threshold over three chunks", [donor, foll], 2.0, (5.0, float(y), 0.0, N, 0.0, 0.0),
                 now=(0.9, 0.8, 1.0, 9.05, 1.05), want={1: {"m": 221, "last_in_c": 128}})
        r = restate(c, [FIXED_ROW], [0])[0][1]
        if np.nonzero(r["in_c"])[0][-1] == 128 and np.abs(r["dist"] - 10.0).min() > 1e-3:
            out.append(c)
            break
    else:
        raise AssertionError("no cyclist position ends the window at sample 128")
    # ---- parameters: every row of the table differs from the next in one launch
    p1 = par(dt=0.05, max_accel=1.0, max_speed=5.0, centerline=0.5, width=1.8, ref_d=6.0, buf_d=1.0, thr_d=2.0, ref_c=5.0, buf_c=1.5, thr_c=1.0, wheelbase=1.2)
    p2 = par(dt=0.2, max_accel=3.0, max_speed=12.0, centerline=-0.3, width=2.2, ref_d=14.0, buf_d=3.0, thr_d=6.0, ref_c=9.0, buf_c=2.5, thr_c=3.0, wheelbase=0.8)
    out.append(case("par: DT 0.05 and every other entry changed", [road[:900], line(700, 0.0171, bend=0.01), mid[:2000]], 1.2, (3.0, -16.0, 1.0, N + 0.03, 0.2, 0.02),
                    now=(0.7, 0.9, 0.8, 1.025, 0.525), p=p1))
    out.append(case("par: DT 0.2 and every other entry changed", [road[:3000], line(2500, 0.0171, bend=0.002), line(900, 0.0171)], 3.0, (3.0, -10.0, 2.0, N - 0.02, -0.1, 0.01),
                    now=(0.7, 0.9, 0.8, 4.1, 2.1), p=p2))
    out.append(case("MAX_ACCEL = 0 at v = 0: no step to resample by", [road[:900], road[:500]], 0.0, _cyclist(), p=par(max_accel=0.0),
                    want={0: {"status": 2}, 1: {"status": 2}}))
    out.append(case("MAX_SPEED = 0: a completion time that is not finite", [mid[:800]], 0.5, _cyclist(), p=par(max_speed=0.0), modes=[1], time_from=[0],
                    want={0: {"status": 2}}))
    # ---- layout
    out.append(case("no candidate", [], 1.0, _cyclist(), modes=[], time_from=[]))
    eight = (20, 63, 65, 127, 130, 255, 258, 310)
    out.append(case("C = 8, every m on another side of 64, 128 and 256", [cut_m(mid, 1, 0.57, RN.DEFAULT_PAR, m) for m in eight], 0.57, _cyclist(3, True),
                    modes=[1] * 8, time_from=list(range(8)), want={k: {"m": m} for k, m in enumerate(eight)}))
    out.append(case("time_from: the donor's nb - 1 = 64, the candidate's own 40", [cut_nb(road, 0, VMAX, RN.DEFAULT_PAR, 65), cut_nb(road, 0, VMAX, RN.DEFAULT_PAR, 41)],
                    VMAX, _cyclist(2), modes=[0, 0], time_from=[0, 0], want={1: {"nb": 65}}))
    # ---- weight rows: P keeps right and passes the cyclist closely, Q gives way to the left
    P, Q = road[:1200], line(1100, 0.0171, bend=0.012)
    out.append(case("ties: bit-identical candidates at 0 / 2 and 1 / 3", [P, Q, P, Q], 1.4, (3.2, -12.0, 1.2, N, 0.0, 0.0), modes=[0] * 4, time_from=list(range(4)),
                    want={"ties": True}))
    out.append(case("a status-2 candidate at index 0", [P[:1], P, Q, mid[:900]], 1.4, (3.2, -12.0, 1.2, N, 0.0, 0.0), want={0: {"status": 2}}))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """The edge situations, every target and margin asserted."""
    out = _build()
    assert len({c["label"] for c in out}) == len(out)
    for c, (res, scores, best) in zip(out, [restate(c) for c in out]):
        modes, _ = layout(c)
        for k, want in c["want"].items():
            if k == "ties":
                assert np.array_equal(scores[:, 0], scores[:, 2]) and np.array_equal(scores[:, 1], scores[:, 3]) and set(best.tolist()) == {0, 1}, c["label"]
                continue
            r = res[k]
            assert r["status"] == want.get("status", 0), (c["label"], k, r["status"])
            if "m" in want:
                assert r["n_samples"] == want["m"], (c["label"], k, r["n_samples"])
            if "n" in want:
                assert len(c["candidates"][k]) == want["n"]
            if "nb" in want:
                assert int(np.ceil(r["ct"] / c["par"][0])) == want["nb"], (c["label"], k, r["ct"] / c["par"][0])
            if "cross" in want:
                assert first_cross(r, c["now"], c["par"]) == want["cross"], (c["label"], first_cross(r, c["now"], c["par"]))
            if "last_in_c" in want:
                assert np.nonzero(r["in_c"])[0][-1] == want["last_in_c"]
        got = margins(c, res, scores)
        assert all(got[k] >= MARGIN[k] for k in MARGIN), (c["label"], got)
    return out


@functools.lru_cache(maxsize=None)
def restated():
    """(per-candidate results, scores [W][C], best [W]) of the restatement for every case under ROWS: computed once, never modified."""
    return [restate(c) for c in cases()]


def index_of(fragment):
    hit = [i for i, c in enumerate(cases()) if fragment in c["label"]]
    assert len(hit) == 1, fragment
    return hit[0]


def sweep_cases():
    """The three situations of the W sweep and of the launch with another ideal."""
    return [index_of("ties:"), index_of("a status-2 candidate"), index_of("m = 129 (mode 1")]


@functools.lru_cache(maxsize=None)
def sweep_rows():
    """1025 weight rows: ROWS first, then a grid of triples that sum to one, forms alternating."""
    trip, _ = RN.weight_triples(0.02)
    w = ROWS_W + trip[3:3 + 1025 - len(ROWS)]
    f = ROWS_F + [k % 2 for k in range(1025 - len(ROWS))]
    assert len(w) == 1025
    return w, f


@functools.lru_cache(maxsize=None)
def restated_sweep():
    out = [restate(cases()[i], *sweep_rows()) for i in sweep_cases()]
    for i, (res, scores, _) in zip(sweep_cases(), out):
        assert margins(cases()[i], res, scores)["top"] >= MARGIN["top"], cases()[i]["label"]
    return out


@functools.lru_cache(maxsize=None)
def restated_ideal():
    out = [restate(cases()[i], ROWS_W, ROWS_F, OTHER_IDEAL) for i in sweep_cases()]
    for i, (res, scores, _) in zip(sweep_cases(), out):
        assert margins(cases()[i], res, scores)["top"] >= MARGIN["top"], cases()[i]["label"]
    return out


def reference_made(c, res):
    """Whether the reference's own functions can make this case: its parameters, its layout, no status, a prediction it can afford."""
    return bool(c["default_par"] and "modes" not in c and len(res) >= 2 and all(r["status"] == 0 and r["nb"] <= REF_MAX_NB for r in res))


def digest(c):
    """The case's inputs as one hash: the fixture's results belong to exactly these numbers."""
    h = hashlib.sha256()
    modes, tf = layout(c)
    for a in c["candidates"] + [np.array(c["ego"]), np.array(c["cyclist"]), np.array(c["now"]), c["par"], np.array(modes, dtype=np.int64), np.array(tf, dtype=np.int64)]:
        h.update(np.ascontiguousarray(a).tobytes())
        h.update(b"|")
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(os.path.join(GOLDEN, "reasons_edges.npz"), allow_pickle=False)


if __name__ == "__main__":
    for i, (c, (res, scores, best)) in enumerate(zip(cases(), restated())):
        m = margins(c, res, scores)
        print(f"{i:2d} {c['label']}: n {[len(t) for t in c['candidates']]} status {[r['status'] for r in res]} m {[r['n_samples'] for r in res]} "
              f"nb {[r.get('nb') for r in res]} cross {[first_cross(r, c['now'], c['par']) for r in res if r['status'] == 0]} best {best.tolist()} "
              f"ref {reference_made(c, res)} margins {' '.join(f'{k} {v:.1e}' for k, v in m.items())}")
