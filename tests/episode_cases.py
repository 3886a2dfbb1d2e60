"""The cases of the per-episode table: one launch that holds every ego of conflict_cases, static_cases and
reason_ticks_cases -- their pose series, flags, vehicles, cyclists and obstacle sets, through their own recorder_arrays -- and
three egos more, with the History columns those helpers leave constant (v, delta, a, xref_deviation) filled in here.  No RNG: each
column is piecewise linear over the 200 ticks, with the knots putting every event where the kernel can go wrong -- 64 ticks per
chunk, an episode carried from chunk to chunk, a row written at the episode's last tick.

Egos: 0-27 conflict_cases (mates keep their batch ranges); 28 `every tick ends an episode` (201 rows; 130 at 129 ticks), 29 `never
ends`, 30 `ends on 60, 130 and on the last record` (an episode over three chunks, a running episode without a tick); 31-59
static_cases; 60-86 reason_ticks_cases.  Every ego meets vehicles, obstacles and a cyclist: its family's own, or, where the family
has none, one picked by its index from another family's."""
import numpy as np

import conflict_cases as TC
import conflicts_numpy as CN
import reason_ticks_cases as RC
import reason_ticks_numpy as TN
from recorder_numpy import AGE, FAILED, GOAL   # noqa: F401
import static_cases as SC
import static_numpy as SN

N = TC.N
TICK_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
EVENT_TICKS = (0, 62, 63, 64, 65, N - 1)               # ego b has its extreme values on EVENT_TICKS[b % 6]
EVERY, NEVER, THREE = 28, 29, 30                       # the three egos that are no family's


def tent(k, lo, hi, end):
    """Piecewise linear: `lo` at tick 0, `hi` at tick k, `end` at the last tick (k at either end: that end holds `hi`)."""
    knots = [(0, lo), (k, hi), (N - 1, end)]
    if k == 0:
        knots = knots[1:]
    elif k == N - 1:
        knots = knots[:2]
    return TC.pw(knots)


def extras():
    h = (-9.0, 0.0, 0.03), (0.011, 0.002, 0.0)
    ego, fl = TC.respawning(*h, list(range(N)))
    out = [TC._case("every tick ends an episode", ego, flags=fl)]
    out.append(TC._case("never ends", TC.line((-20.0, 0.13, 0.02), (19.8, 0.13, 0.02))))
    ego, fl = TC.respawning(*h, [60, 130, N - 1])
    out.append(TC._case("ends on 60, 130 and on the last record", ego, flags=fl))
    return out


def history_columns(b, flags_b):
    """v, delta, a, xref_deviation [N] of ego b and its flags with the FAILED bits."""
    K = EVENT_TICKS[b % 6]
    v = tent(K, 2.0, 9.0, 2.5)                                         # the largest speed on tick K
    a = tent(K, -0.4, 1.8, -1.1 - 0.01 * b)                            # the largest acceleration on K, the smallest on the last tick
    delta = tent(K, 0.05, -0.6, 0.2)                                   # the largest |delta| on K, with a negative sign
    dev = tent(K, 0.1, 1.4, 0.3)
    if K == N - 1:
        a[0] = -2.0                                                    # (the smallest on tick 0 then)
    if b % 5 == 1:        # the same extreme value twice, in different chunks: the first one wins
        v[[10, 150]] = 11.0
        dev[[30, 100]] = 7.0
        a[[20, 140]] = -3.0
        a[[50, 70]] = 2.5
    if b % 7 == 2:        # a NaN deviation on some ticks, across a chunk edge and on an extreme tick
        dev[[5, 6, 7, 8, 9, 63, 64, K]] = np.nan
    fl = np.array(flags_b, dtype=np.int32)
    if b % 4 == 0:        # FAILED on both sides of a chunk edge
        fl[[62, 63, 64, 65]] |= FAILED
    elif b % 4 == 1:
        fl[[0, 127, 128, N - 1]] |= FAILED
    # a NaN deviation on every tick of one episode
    if b == 13:           # conflict case 13: the episode 0 .. 62
        dev[:63] = np.nan
    if b == 16:           # conflict case 16: the episode of one tick, 101
        dev[101] = np.nan
    if b == EVERY:
        dev[::3] = np.nan
    return v, delta, a, dev, fl


def recorder_arrays():
    """The launch: rec [N][B][7], flags [N][B], obs [N][n_obs][6], x_first, x_spawn [B][4] and the arguments of the three
    evaluations: veh_range, mate_range, shapes (conflicts); set_of with the static fixture's tables (static); veh_of, par, threshold,
    carry (reasons)."""
    fam = [TC.recorder_arrays(TC.cases() + extras()), SC.recorder_arrays(SC.cases()), RC.recorder_arrays(RC.cases())]
    sizes = [f["rec"].shape[1] for f in fam]
    assert sizes == [31, 29, 27]
    B = sum(sizes)
    cat = lambda k, axis: np.concatenate([f[k] for f in fam], axis=axis)
    A = {"rec": cat("rec", 1), "flags": cat("flags", 1), "x_first": cat("x_first", 0), "x_spawn": cat("x_spawn", 0)}
    n_c, n_r = fam[0]["obs"].shape[1], fam[2]["obs"].shape[1]
    A["obs"] = np.concatenate([fam[0]["obs"], fam[2]["obs"]], axis=1)
    A["shapes"] = np.concatenate([fam[0]["shapes"], np.tile(np.array([[*TC.BIKE, 1.0]]), (n_r, 1))])
    j = np.arange(B - sizes[0])
    other = 1 + j % (n_c - 1)                                          # (vehicle 0 is the decoy)
    A["veh_range"] = np.concatenate([fam[0]["veh_range"], np.stack([other, other + 1], axis=1)]).astype(np.int32)
    me = np.arange(sizes[0], B)
    A["mate_range"] = np.concatenate([fam[0]["mate_range"], np.stack([me, me], axis=1)]).astype(np.int32)
    n_sets = len(SC.SET_NAMES)
    A["set_of"] = np.concatenate([np.arange(sizes[0]) % n_sets, fam[1]["set_of"], np.arange(sizes[2]) % n_sets]).astype(np.int32)
    rv = fam[2]["veh_of"]
    A["veh_of"] = np.concatenate([n_c + 1 + np.arange(sizes[0] + sizes[1]) % (n_r - 1), np.where(rv >= 0, n_c + rv, -1)]).astype(np.int32)
    A["par"] = np.concatenate([np.tile(RC.par_row(), (sizes[0] + sizes[1], 1)), fam[2]["par"]])
    A["threshold"] = np.concatenate([np.full(sizes[0] + sizes[1], TN.THRESHOLD), fam[2]["threshold"]])
    A["carry"] = np.concatenate([np.zeros((sizes[0] + sizes[1], 3)), fam[2]["carry"]])
    for b in range(B):
        v, delta, a, dev, fl = history_columns(b, A["flags"][:, b])
        A["rec"][:, b, 3], A["rec"][:, b, 4], A["rec"][:, b, 5], A["rec"][:, b, 6], A["flags"][:, b] = v, delta, a, dev, fl
    return A


def per_tick(A, n=N, w=0, hidden=0):
    """The three evaluations' per-tick outputs on the first n ticks, by their restatements: (veh, st, rs) as the summary takes them."""
    if n == 0:            # (the restatements take at least one tick)
        B = A["rec"].shape[1]
        f, i = (lambda *sh: np.zeros((0, B, *sh))), (lambda: np.zeros((0, B), dtype=np.int32))
        return ({"clear": f(), "who": i(), "hit_tick": i(), "hit_frame": i(), "hit_xy": f(2)},
                {"clear": f(), "who": i(), "hit": i(), "off_tick": i()}, {"val": f(4), "trig": i()})
    g = SC.fixture()
    rec, flags, obs, xf, xs = A["rec"][:n], A["flags"][:n], A["obs"][:n], A["x_first"], A["x_spawn"]
    veh = CN.eval_conflicts(rec, flags, obs, xf, xs, A["veh_range"], A["mate_range"], A["shapes"], TC.CAR, w)
    st = SN.eval_static(rec, flags, xf, xs, A["set_of"], g["set_off"], g["rows"], SC.CAR, bool(hidden))
    rs = TN.eval_ticks(rec, flags, obs, xf, xs, A["veh_of"], A["par"], A["threshold"], A["carry"])
    return ({k: veh[k] for k in ("clear", "who", "hit_tick", "hit_frame", "hit_xy")}, {k: st[k] for k in ("clear", "who", "hit", "off_tick")},
            {"val": rs["val"], "trig": rs["trig"]})
