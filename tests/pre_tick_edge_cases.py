"""Edge cases of the collision cut-off glue (jsim_pre_tick_ego, csrc/loop_pre_tick.inc) as data: situations chosen
for the kernel's structure -- 64-point chunks with a carried running sum and a carried floor, 8-frame blocks, a mixed-radix row counter
stepped by 32 pairs per 64 rows, a bounding-circle cull that compacts the obstacle list, a packed key whose minimum is the first row,
and the tables' limits (320 resampled points, 8 obstacles, 64 predicted steps, frame_window 32) -- not for the reference's behaviour.

Every case is deterministic: synthetic paths (straight lines, an arc, a closed loop driven twice), stationary or straight-moving
obstacles.  Where a position is found by a search it is a fixed scan over a grid (scan(), tie_offset()), no RNG.  A case says what it
is meant to be in `want` (n_res, status, frame and row of the first hit, R, culled obstacles, clamp ...); tests/test_pre_tick_edges_cpu.py
asserts all of it with the restatement, so a case that stops being what its label says fails there.

run(c) is the glue restated from the pieces of oracle/loop_oracle.py and tests/shapes_numpy.py with the pair table written out
([frame, ego circle, obstacle, offset, obstacle circle]) so that the first row, R, the margins and the mutants of the CPU test can be
read off it; the CPU test pins it to shapes_numpy.loop_pre_tick / first_collision / first_collision_fast on every case.  Nothing here
is a new statement of the reference: run() without mutants IS loop_pre_tick plus the table limit (status 4 above 320 points)."""
import functools
import hashlib
import math
import os

import numpy as np

import loop_oracle as LO
import shapes_numpy as SN
from conftest import GOLDEN

DT, VMAX, AMAX = LO.DT, LO.MAX_SPEED, LO.MAX_ACCEL
CAR, BIKE = SN.shape_of(), SN.shape_of(*SN.BIKE)
BIKE_DIMS = dict(L=SN.BIKE[0], width=SN.BIKE[1], extra_length=SN.BIKE[2])
EGO_R, EGO_OFFS = LO.car_circles(2.86)
MAX_RES, MAX_OBS, MAX_PRED, MAX_W = 320, 8, 64, 32
STATUS_TABLE = 4                                  # the resampled path outgrew the kernel's table
MARGIN = 1e-9                                     # every tested distance of a case that is no exact tie is this far from its threshold
MUTANTS = ("tree_cumsum", "kprev_not_carried", "lt_for_le", "thr_times_thr", "rows_o_before_a", "block_min_without_frame",
           "no_clamp_low", "no_clamp_high", "o_compacted", "mm_search_from_idx", "rear_circle_first")
UP = math.pi / 2


# ------------------------------------------------------------------------------------------------ paths and vehicles
def straight(n, spacing=2.0, x0=0.0, y=0.0):
    """n points along +x, yaw 0 (cos = 1, sin = 0 exactly on host and device)."""
    return np.stack([x0 + np.arange(n) * spacing, np.full(n, y), np.zeros(n)], 1)


def arc(n, spacing, radius):
    s = np.arange(n) * spacing / radius
    return np.stack([radius * np.sin(s), radius * (1.0 - np.cos(s)), s], 1)


def twice_round(per_lap, radius):
    """A closed loop driven twice: the second lap retraces the first point for point."""
    th = np.arange(per_lap) * (2 * math.pi / per_lap)
    lap = np.stack([radius * np.cos(th), radius * np.sin(th), th + UP], 1)
    return np.tile(lap, (2, 1))


def cumsum_line(n, frac):
    """x = cumsum of n equal steps DT * MAX_SPEED / frac: a sequential and a tree-order prefix sum round differently on it."""
    return np.stack([np.cumsum(np.full(n, DT * VMAX / frac)), np.zeros(n), np.zeros(n)], 1)


def parked(x, y, yaw=0.0):
    return (float(x), float(y), 0.0, float(yaw), 0.0, 0.0)


def blocker(f, side=1.0, lateral=2.5):
    """A parked car beside a 2 m path along y = 0 whose REAR circle the ego's FRONT circle first touches at path point f."""
    return parked(2.0 * f + 2.0, side * lateral)


def crossing(x, f, speed=20.0, reach=-2.5, shape=CAR):
    """A vehicle driving up (+y) at constant x whose front circle stands at y = reach in predicted sample f (4 m per sample at 20 m/s)."""
    return (float(x), reach - shape[0] - speed * DT * (f + 1), float(speed), UP, 0.0, 0.0)


FAR = parked(900.0, 700.0)


# ------------------------------------------------------------------------------------------------ the glue, restated with its table
def horizon_of(n_steps):
    """A time_horizon that PreTick and np.arange(0, horizon, DT) both turn into n_steps."""
    return n_steps * DT - DT / 2


def predictions(c):
    p = [LO.predict_obstacle(*o, dt=DT, L=sh[3], horizon=horizon_of(c["n_steps"])) for o, sh in zip(c["obst"], c["shapes"])]
    assert all(len(q) == c["n_steps"] for q in p)
    return p


def tree_cumsum(step):
    """A 64-lane tree-order (Hillis-Steele) inclusive prefix sum per chunk, the chunk's carry added last."""
    out, carry = np.empty_like(step), 0.0
    for b in range(0, len(step), 64):
        x = np.zeros(64)
        x[:len(step[b:b + 64])] = step[b:b + 64]
        d = 1
        while d < 64:
            y = x.copy()
            y[d:] = x[d:] + x[:-d]
            x, d = y, 2 * d
        m = len(step[b:b + 64])
        out[b:b + m] = carry + x[:m]
        carry = out[b + m - 1]
    return out


def resample_mask(xy, dl, mut=()):
    """loop_oracle.resample_mask; mutants: the cumulative sum in tree order, the previous floor not carried into a chunk's lane 0."""
    n = len(xy)
    step = np.zeros(n)
    d = xy[1:] - xy[:-1]
    step[1:] = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    cum = tree_cumsum(step) if "tree_cumsum" in mut else np.cumsum(step)
    k = np.floor(cum / dl).astype(np.int64)
    kp = np.append(0, k[:-1])
    if "kprev_not_carried" in mut:
        kp[64::64] = 0
    mask = (k - kp) >= 1
    mask[0] = mask[-1] = True
    return mask


def bounding_circle(cc):
    """The circle the kernels put around a set of circle centres: the box's middle, the largest distance from it, inflated."""
    mx, my = 0.5 * (cc[:, 0].min() + cc[:, 0].max()), 0.5 * (cc[:, 1].min() + cc[:, 1].max())
    dx, dy = cc[:, 0] - mx, cc[:, 1] - my
    return mx, my, float(np.sqrt(dx * dx + dy * dy).max()) * (1.0 + 1e-9) + 1e-9


def culled(res, preds, shapes):
    """Obstacles the bounding-circle test drops: their circle and the ego's stay further apart than the pair's threshold."""
    ex, ey, er = bounding_circle(np.concatenate([LO.circle_centres(res, xo) for xo in EGO_OFFS]))
    out = []
    for o, (p, sh) in enumerate(zip(preds, shapes)):
        ox, oy, orad = bounding_circle(np.concatenate([LO.circle_centres(p, xo) for xo in sh[:2]]))
        if not math.sqrt((ox - ex) * (ox - ex) + (oy - ey) * (oy - ey)) - orad - er <= EGO_R + sh[2]:
            out.append(o)
    return out


def sqrt_threshold(thr):
    """The largest double whose square root is <= thr."""
    x = thr * thr
    while math.sqrt(x) > thr:
        x = np.nextafter(x, 0.0)
    while math.sqrt(np.nextafter(x, np.inf)) <= thr:
        x = np.nextafter(x, np.inf)
    return float(x)


def pair_table(res, preds, shapes, w, mut=()):
    """(d2 [F, a, o, off, b], touch mask, obstacle points [F, o, off, b, 2], thr [o]) in the reference's row order.  Mutants without a
    clamp read the flat [o][sample] table past the obstacle's own samples, as an unclamped index would."""
    P, no = len(preds[0]), len(preds)
    F = max(len(res), P)
    fa, fo = np.minimum(np.arange(F), len(res) - 1), np.minimum(np.arange(F), P - 1)
    j = fo[:, None] - np.arange(-w, w + 1)[None, :]
    lo, hi = (-10 ** 9 if "no_clamp_low" in mut else 0), (10 ** 9 if "no_clamp_high" in mut else P - 1)
    j = np.clip(j, lo, hi)
    ego = np.stack([LO.circle_centres(res, xo)[fa] for xo in EGO_OFFS], axis=1)                    # [F, a, 2]
    flat = np.stack([np.stack([LO.circle_centres(p, xo) for xo in sh[:2]], axis=1) for p, sh in zip(preds, shapes)]).reshape(no * P, 2, 2)
    at = np.arange(no)[None, :, None] * P + j[:, None, :]                                          # [F, o, off] into [o * P + sample]
    inside = (at >= 0) & (at < no * P)
    obs = np.where(inside[..., None, None], flat[np.clip(at, 0, no * P - 1)], np.inf)              # [F, o, off, b, 2]
    thr = np.array([EGO_R + sh[2] for sh in shapes])
    d = ego[:, :, None, None, None, :] - obs[:, None]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    t = thr[None, None, :, None, None]
    with np.errstate(invalid="ignore"):
        if "thr_times_thr" in mut:
            touch = d2 <= t * t
        elif "lt_for_le" in mut:
            touch = np.sqrt(d2) < t
        else:
            touch = np.sqrt(d2) <= t
    return d2, touch, obs, thr


def first_row(touch, mut=()):
    """(frame, a, o, offset index, b) of the first touching row, or None.  Mutants: obstacle-major rows; the minimum of an 8-frame
    block taken over the row number alone (the latest such frame's, as a key without the frame would leave it)."""
    if not touch.any():
        return None
    if "rows_o_before_a" in mut:
        f, o, a, k, b = np.unravel_index(int(np.argmax(touch.transpose(0, 2, 1, 3, 4).reshape(-1))), touch.transpose(0, 2, 1, 3, 4).shape)
        return int(f), int(a), int(o), int(k), int(b)
    if "block_min_without_frame" in mut:
        F = touch.shape[0]
        rows = touch.reshape(F, -1)
        for f0 in range(0, F, 8):
            blk = rows[f0:f0 + 8]
            if blk.any():
                r = int(np.argmax(blk.any(axis=0)))
                f = f0 + int(np.argmax(blk[:, r]))
                return (f,) + tuple(int(v) for v in np.unravel_index(r, touch.shape[1:]))
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(touch.reshape(-1))), touch.shape))


def run(c, mut=()):
    """One ego's glue: dict(status, traj_idx, n_res, kept, hit, first_idx, col_xy, path_len, row, R, culled, margin).  A status
    leaves traj_idx / path_len as they came in (path_len None: whatever the buffer held)."""
    import oracle_py as O
    full, (x, y, v, yaw) = c["path"], c["state"]
    M, idx, prev = len(full), c["idx"], c["prev"]
    out = dict(status=0, traj_idx=idx, n_res=-1, kept=np.zeros(0, dtype=np.int64), hit=False, first_idx=-1, col_xy=(0.0, 0.0),
               path_len=None, row=None, R=0, culled=[], margin=np.inf)
    if prev < 0 or idx != prev - 1:
        st, k = O.nearest_index_in_direction(x, y, full[:, 0], full[:, 1], idx, True)
        if st != 0:
            return dict(out, status=st)
        idx = k
    detailed = full[idx:]
    mask = resample_mask(detailed[:, :2], LO.ego_resample_dl(len(detailed), v, DT), mut)
    kept = np.flatnonzero(mask)
    if len(kept) > MAX_RES:
        return dict(out, status=STATUS_TABLE, n_res=len(kept))
    res = detailed[mask]
    out.update(traj_idx=idx, n_res=len(kept), kept=kept, path_len=M)
    if not c["obst"]:
        return out
    preds, shapes, w = predictions(c), c["shapes"], c["w"]
    gone = culled(res, preds, shapes)
    d2, touch, obs, thr = pair_table(res, preds, shapes, w, mut)
    assert mut or not touch[:, :, gone].any(), c["label"]             # the cull never drops an obstacle that touches
    out.update(culled=gone, R=4 * (len(preds) - len(gone)) * (2 * w + 1))
    row = first_row(touch, mut)
    gap = np.abs(np.sqrt(d2) - thr[None, None, :, None, None]).reshape(-1)
    if row is None:
        out["margin"] = float(gap.min())
        return out
    f, a, o, k, b = row
    out["margin"] = float(gap[:int(np.ravel_multi_index(row, touch.shape)) + 1].min())
    o_hit = o
    if "o_compacted" in mut:
        o_hit = [q for q in range(len(preds)) if q not in gone].index(o)
    hit = obs[f, o_hit, k, b]
    first = 0
    for aa in ((1, 0) if "rear_circle_first" in mut else (0, 1)):
        cc = LO.circle_centres(detailed, EGO_OFFS[aa])
        dx, dy = hit[0] - cc[:, 0], hit[1] - cc[:, 1]
        dist = np.sqrt(dx * dx + dy * dy)
        out["margin"] = min(out["margin"], float(np.abs(dist - thr[o]).min()))
        if (dist <= thr[o]).any():
            first = int(np.argmax(dist <= thr[o]))
            break
    cx, cy = float(detailed[first, 0]), float(detailed[first, 1])
    start = idx if "mm_search_from_idx" in mut else 0
    dx, dy = full[start:, 0] - cx, full[start:, 1] - cy
    dist = np.sqrt(dx * dx + dy * dy)
    out["margin"] = min(out["margin"], float(np.abs(dist - 0.001).min()))
    cidx = start + int(np.argmax(dist <= 0.001))
    margin = c["margin_factor"] * int(math.ceil(EGO_R / c["dl"]))
    P = len(preds[0])
    j = min(max(min(f, P - 1) - (k - w), 0), P - 1)
    out.update(hit=True, first_idx=first, col_xy=(cx, cy), path_len=max(idx + 1, cidx - margin), row=(f, a, o, k - w, b), sample=j)
    return out


# ------------------------------------------------------------------------------------------------ cases
def case(label, path, v, obst=(), shapes=None, w=10, n_steps=35, idx=0, dl=None, mf=4, prev="pin", state=None, tie=False,
         ref=None, **want):
    path = np.ascontiguousarray(path, dtype=np.float64)
    obst = [tuple(float(q) for q in o) for o in obst]
    shapes = [CAR] * len(obst) if shapes is None else list(shapes)
    assert len(shapes) == len(obst) <= MAX_OBS and 0 <= w <= MAX_W and 1 <= n_steps <= MAX_PRED
    if dl is None:
        dl = float(np.hypot(*(path[1, :2] - path[0, :2]))) if len(path) > 1 else 2.0
    if state is None:
        state = (path[idx, 0], path[idx, 1], v, path[idx, 2])
    return dict(label=label, path=path, state=tuple(float(q) for q in state), idx=int(idx), prev=int(idx + 1 if prev == "pin" else prev),
                obst=obst, shapes=shapes, w=int(w), n_steps=int(n_steps), dl=float(dl), margin_factor=int(mf), tie=bool(tie),
                ref=ref, want=want)


def scan(make, grid, ok):
    """The first value of `grid` whose case `ok` accepts (restated, with the input margin kept)."""
    for g in grid:
        c = make(g)
        r = run(c)
        if r["margin"] >= 10 * MARGIN and ok(r):
            return c
    raise AssertionError("no grid value gives the wanted case: " + make(grid[0])["label"])


def tie_offset(shape, up):
    """(X, Y) of a parked vehicle of `shape` (yaw 0) whose FRONT circle lies at a squared distance from the REAR circle of path point
    (0, 0) that is exactly the largest double with a square root <= thr (up = 0: touches) or the next double (up = 1: does not).
    A fixed scan over Y on a 2^-20 grid and X over neighbouring doubles; dx ~ -0.3, so no other circle pair comes near."""
    thr = EGO_R + shape[2]
    target = sqrt_threshold(thr)
    if up:
        target = float(np.nextafter(target, np.inf))
    ego = LO.circle_centres(np.zeros((1, 3)), EGO_OFFS[1])[0]
    for ky in range(4096):
        Y = math.sqrt(thr * thr - 0.09) + ky * 2.0 ** -20
        X0 = ego[0] + math.sqrt(max(target - Y * Y, 0.0)) - shape[0]
        X = X0
        for _ in range(64):
            X = float(np.nextafter(X, -np.inf))
        for _ in range(128):
            po = LO.circle_centres(np.array([[X, Y, 0.0]]), shape[0])[0]
            dx, dy = ego[0] - po[0], ego[1] - po[1]
            if dx * dx + dy * dy == target:
                return X, Y
            X = float(np.nextafter(X, np.inf))
    raise AssertionError("no exact tie found")


def _resampling():
    out = []
    for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 640):
        out.append(case(f"fine path of {n} points", straight(n, 0.1), 3.0, [parked(6.0, 2.5)] if n > 60 else []))
    dl = DT * VMAX
    out.append(case("kept point on lane 0 of the second chunk", straight(130, dl * 5 / 63.5), VMAX, keeps=(64,), drops=(63, 65)))
    out.append(case("kept point on lane 63 of the first chunk", straight(130, dl * 5 / 62.5), VMAX, keeps=(63,), drops=(62, 64)))
    out.append(case("v = 0", straight(640, 0.1), 0.0, [parked(40.0, 2.5)], hit=True))
    out.append(case("speed limit reached inside the second chunk", straight(200, 0.1), VMAX - 199.5))
    out.append(case("v = MAX_SPEED exactly", straight(300, 0.1), VMAX, [parked(20.0, -2.5)], hit=True))
    out.append(case("v above MAX_SPEED", straight(300, 0.1), 10.0, [parked(20.0, -2.5)], hit=True))
    out.append(case("n_res = 1 at the path's end", straight(5), VMAX, idx=4, n_res=1))
    for m in (2, 64, 65, 128, 129, 319, 320):
        out.append(case(f"n_res = {m}", straight(m), VMAX, [blocker(min(5, m - 1))] if m > 2 else [], n_res=m, status=0))
    out.append(case("320 of 321 points kept at v = 0", straight(321), 0.0, [blocker(7)], n_res=320, status=0, hit=True))
    out.append(case("321 of 322 points kept at v = 0: refused", straight(322), 0.0, [blocker(7)], ref=False, n_res=321, status=STATUS_TABLE))
    out.append(case("n_res = 321: refused", straight(321), VMAX, [blocker(5)], ref=False, n_res=321, status=STATUS_TABLE))
    out.append(case("n_res = 700: refused", straight(700), VMAX, [blocker(5)], ref=False, n_res=700, status=STATUS_TABLE))
    for frac, v in ((1, 0.0), (2, 5.0), (3, VMAX), (5, 0.0), (5, VMAX)):
        out.append(case(f"order-sensitive cumulative sum, step / {frac}, v = {v:.3g}", cumsum_line(300, frac), v, dl=DT * VMAX / frac,
                        order_sensitive=True))
    return out


def _pair_table():
    out = []
    near = [parked(10.0 + 9 * k, (-1) ** k * 4.6) for k in range(7)]               # within reach of the bounding circles, never touching
    for w, no in ((0, 1), (1, 2), (2, 5), (10, 8), (15, 1), (16, 2), (31, 5), (32, 8)):
        for ns in ((35,) if w not in (31, 32) else (35, 64)):
            mk = lambda f, w=w, no=no, ns=ns: case(f"frame_window {w}, {no} obstacles, {ns} steps", straight(40), VMAX,   # noqa: E731
                                                   near[:no - 1] + [crossing(30.68, f, speed=8.0)], w=w, n_steps=ns, R=4 * no * (2 * w + 1))
            out.append(scan(mk, range(8, 34), lambda r: r["hit"] and not r["culled"]))
    # a first hit in frame 0, 7, 8, 9 and F - 1, F = n_res > n_steps (the obstacle's sample index clamps) ...
    out.append(case("first hit in frame 0 of F = n_res = 20 > n_steps = 5", straight(20), VMAX, [blocker(0)], w=0, n_steps=5, frame=0))
    for f in (7, 8, 9, 19):                       # the vehicle stands where its last sample left it
        mk =lambda x, f=f: case(f"first hit in frame {f} of F = n_res = 20 > n_steps = 5", straight(20), VMAX,      # noqa: E731
                                 [crossing(x, 4, speed=10.0, reach=-0.8)], w=0, n_steps=5, frame=f)
        out.append(scan(mk, np.arange(0.0, 48.0, 0.25), lambda r, f=f: r["hit"] and r["row"][0] == f))
    # ... and F = n_steps = 35 > n_res = 12 (the ego's index clamps): the vehicle arrives beside the ego's last point in sample f
    for f in (0, 7, 8, 9, 34):
        if f < 11:
            c = case(f"first hit in frame {f} of F = n_steps = 35 > n_res = 12", straight(12), VMAX, [blocker(f)], w=0, frame=f)
        else:
            c = case(f"first hit in frame {f} of F = n_steps = 35 > n_res = 12", straight(12), VMAX, [crossing(22.68, f)], w=0, frame=f,
                     row=(f, 1, 0, 0, 0))
        out.append(c)
    out.append(case("hit only through the -w copy, on the last sample", straight(5), VMAX, [crossing(8.68, 34)], w=10, row=(24, 1, 0, -10, 0),
                    sample=34))
    out.append(case("hit only through the +w copy, on sample 0", straight(40), VMAX, [crossing(2.0 * 5 + 2.68, 0, reach=4.0)], w=5, row=(5, 0, 0, 5, 1),
                    sample=0))
    out.append(case("ego's rear circle only", straight(30), VMAX, [parked(-2.0, 2.5)], w=3, row=(0, 1, 0, -3, 0)))
    out.append(case("obstacle's rear circle only", straight(30), VMAX, [blocker(6)], w=3, row=(6, 0, 0, -3, 1)))
    out.append(case("two rows touch in one frame: (a, o) order decides", straight(30), VMAX, [crossing(2.0 * 4 + 0.68, 4), blocker(4, side=1.0)],
                    w=0, row=(4, 0, 1, 0, 1), first_idx=4))
    out.append(case("two rows touch in one 8-frame block: the earlier frame wins", straight(30), VMAX, [blocker(5), crossing(2.0 * 2 + 0.68, 2)],
                    w=0, row=(2, 1, 1, 0, 0), first_idx=1))
    out.append(case("an unclamped sample index would read the next obstacle", straight(30), VMAX, [parked(30.0, -4.6), parked(2.0 * 3 + 2.0 + 0.775, 2.1)],
                    [CAR, BIKE], w=4, n_steps=3, hit=False))
    out.append(case("an unclamped sample index would read the previous obstacle", straight(30), VMAX, [parked(2.0 * 3 + 2.0 + 0.775, 2.1), parked(30.0, -4.6)],
                    [BIKE, CAR], w=4, n_steps=3, hit=False))
    for ns, w in ((1, 0), (1, 1), (2, 1), (2, 2), (1, 10), (2, 10), (63, 10), (64, 10), (64, 32)):
        out.append(case(f"n_steps = {ns}, frame_window {w}", straight(30), VMAX, [parked(70.0, 4.6), blocker(3)], w=w, n_steps=ns, hit=True))
    return out


def _cull_and_thresholds():
    out = [case("a culled obstacle between two near ones, hit on the one after it", straight(30), VMAX, [parked(20.0, -4.6), FAR, blocker(6)],
                culled=[1], row=(6, 0, 2, -10, 1), first_idx=6),
           case("obstacle 0 culled", straight(30), VMAX, [FAR, blocker(4)], culled=[0], row=(4, 0, 1, -10, 1)),
           case("all eight culled", straight(30), VMAX, [parked(900.0 + 50 * k, 700.0) for k in range(8)], culled=list(range(8)), hit=False, R=0),
           case("only contact at the far end of the ego's path, on its last point", straight(30), VMAX, [blocker(29)], row=(29, 0, 0, -10, 1),
                first_idx=29)]
    bike_blocker = lambda f: parked(2.0 * f + 2.0 + 0.68 + 0.095, 1.5)              # noqa: E731  its rear circle where a car blocker's is
    out.append(case("cyclists only", straight(30), VMAX, [parked(30.0, -3.0), bike_blocker(4)], [BIKE, BIKE], mf=2, hit=True))
    out.append(case("a cyclist and a car at the same lateral distance: only the car touches", straight(30), VMAX,
                    [parked(2.0 * 3 + 2.0 + 0.775, 2.1), parked(2.0 * 6 + 2.0, 2.1), parked(40.0, -1.5)], [BIKE, CAR, BIKE], row=(6, 0, 1, -10, 1)))
    out.append(case("mixed shapes, the cyclist is hit", straight(30), VMAX, [parked(2.0 * 9 + 2.0, -2.5), bike_blocker(5)], [CAR, BIKE], w=2, hit=True,
                    first_idx=5))
    for name, shape in (("car", CAR), ("cyclist", BIKE)):
        for up in (0, 1):
            X, Y = tie_offset(shape, up)
            out.append(case(f"exact tie at the {name} threshold, {'next double up: no touch' if up else 'touches'}", straight(3), VMAX, [parked(X, Y)],
                            [shape], w=0, tie=True, hit=not up, **({} if up else dict(row=(0, 1, 0, 0, 0)))))
    return out


def _cutoff():
    fine = straight(400, 0.1)
    loop = twice_round(200, 10.0)
    ahead = loop[260]
    return [case("cut-off clamped to idx + 1", fine, 4.0, [parked(5.0 + 3.0, 2.5)], idx=50, clamp=True),
            case("margin factor 4", fine, 4.0, [parked(30.0, 2.5)], idx=20, mf=4, clamp=False, hit=True),
            case("margin factor 2, cyclist", fine, 4.0, [parked(30.0, 1.5)], [BIKE], idx=20, mf=2, clamp=False, hit=True),
            case("second lap of a closed loop: the 1 mm search finds the first lap", loop, 3.0,
                 [parked(ahead[0] * 1.25, ahead[1] * 1.25, ahead[2])], idx=220, clamp=True, second_lap=True),
            case("an arc", arc(300, 0.1, 15.0), 2.0, [parked(14.0, 12.0, 1.2)], idx=10, hit=True),
            case("detailed path of one point, touched", straight(5), 0.0, [parked(8.0 + 1.5, 2.5)], idx=4, n_res=1, row=(0, 0, 0, -10, 1), path_len=5)]


def _progress():
    out = []
    for left in (2, 3, 63, 64, 65, 129):
        M = left + 7
        p = straight(M, 0.5)
        k = 7 + min(left - 1, 4)
        out.append(case(f"progress index with {left} points left", p, 2.0, idx=7, prev=-1, state=(p[k, 0] + 0.2, 0.3, 2.0, 0.0)))
    p = straight(200, 0.5)
    out.append(case("nearest point on lane 0 of the second chunk", p, 2.0, idx=10, prev=-1, state=(p[74, 0] + 0.2, -0.3, 2.0, 0.0), traj_idx=74))
    out.append(case("nearest point on lane 63 of the first chunk", p, 2.0, idx=10, prev=5, state=(p[73, 0] + 0.2, -0.3, 2.0, 0.0), traj_idx=73))
    out.append(case("equal distances to the first two points", p, 2.0, idx=10, prev=-1, state=(p[10, 0] + 0.25, 0.0, 2.0, 0.0), traj_idx=11))
    u = np.concatenate([straight(20, 0.5), np.stack([np.full(10, 12.0), np.linspace(0.1, 0.9, 10), np.full(10, UP)], 1), straight(20, -0.5, x0=9.5, y=1.0)])
    out.append(case("nearest-three anomaly: status, nothing written", u, 2.0, [parked(6.0, 3.0)], idx=0, prev=-1, state=(2.5, 0.45, 2.0, 0.0), ref=False,
                    status=2, dl=0.5))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _resampling() + _pair_table() + _cull_and_thresholds() + _cutoff() + _progress()
    assert len({c["label"] for c in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def restated():
    return [run(c) for c in cases()]


def reference_made(c, r):
    """The reference's own functions can make the case: one shape for all obstacles, frame_window <= n_steps, no status."""
    if c["ref"] is not None:
        return c["ref"]
    return r["status"] == 0 and len(set(c["shapes"])) <= 1 and c["w"] <= c["n_steps"]


def launch_key(c):
    """Cases that can share one launch of loop_pre_tick_kernel: everything that is per launch, not per ego."""
    return (c["w"], c["n_steps"], tuple(c["obst"]), tuple(c["shapes"]), c["dl"], c["margin_factor"])


def launches():
    """[(key, [case indices])] in first-appearance order."""
    groups = {}
    for i, c in enumerate(cases()):
        groups.setdefault(launch_key(c), []).append(i)
    return list(groups.items())


def digest(c):
    h = hashlib.sha256()
    for a in (c["path"], np.array(c["state"]), np.array([c["idx"], c["prev"], c["w"], c["n_steps"], c["margin_factor"]], dtype=np.int64),
              np.array(c["obst"], dtype=np.float64).reshape(-1, 6), np.array(c["shapes"], dtype=np.float64).reshape(-1, 4), np.array([c["dl"]])):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(os.path.join(GOLDEN, "pre_tick_edges.npz"), allow_pickle=False))


def expected(i):
    """Entry i of the fixture as run() returns it (what a device run must equal): the cases, then the egos of the group cases."""
    g = fixture()
    return dict(status=int(g["status"][i]), traj_idx=int(g["traj_idx"][i]), n_res=int(g["n_res"][i]), kept=g["kept"][g["kept_off"][i]:g["kept_off"][i + 1]],
                hit=bool(g["hit"][i]), first_idx=int(g["first_idx"][i]), col_xy=tuple(float(v) for v in g["col_xy"][i]),
                path_len=int(g["path_len"][i]), row=tuple(int(v) for v in g["row"][i]), digest=str(g["digest"][i]), ref_made=bool(g["ref_made"][i]))


# ------------------------------------------------------------------------------------------------ interacting groups
def _lane(x0, y, n=24):
    return straight(n, 2.0, x0=x0, y=y)


def arterial(x, y, speed=0.0, dims=None):
    d = dict(kind="arterial", x_init=float(x), y_init=float(y), speed=float(speed), initial_speed=float(speed), offset=None)
    if dims is not None:
        d["dims"] = dims
    return d


@functools.lru_cache(maxsize=None)
def group_cases():
    """Three InteractingLoop first ticks: every ego stands (v = 0) on point 0 of its own straight 2 m path; the scripted vehicles are
    parked arterial ones.  dict(label, paths, x0 [B, 4] (x, y, v, yaw), sizes, specs, w)."""
    out = []
    # 0 scripted + a group of 8: two columns of lanes 2.5 m apart, staggered so that each of the last four egos meets one of the first four ahead
    paths = [_lane(2.0 * (7 + k) + 2.0, 40.0 * k + 2.5) for k in range(4)] + [_lane(0.0, 40.0 * k) for k in range(4)]
    out.append(dict(label="no scripted vehicle, a group of 8", paths=paths, sizes=[8], specs=[], w=20, hit_o={4: 0, 5: 1, 6: 2, 7: 3}))
    # 7 scripted + a group of 2: a scripted vehicle and the mate touch in the same frame of ego 0 (the scripted one wins)
    paths = [_lane(0.0, 0.0), _lane(2.0 * 9 + 2.0, 2.5)]
    specs = [arterial(100.0 + 9 * k, -4.6) for k in range(6)] + [arterial(2.0 * 9 + 2.0 + 2.18, -2.5 - 0.68)]
    out.append(dict(label="7 scripted vehicles, a group of 2", paths=paths, sizes=[2], specs=specs, w=20, hit_o={0: 6}, also={0: 7}))
    # 3 scripted (one a cyclist at 2.0 m that only a car would touch) + a group of 4: only a mate touches, by the mates' threshold
    paths = [_lane(0.0, 0.0), _lane(2.0 * 7 + 2.0, 2.1), _lane(0.0, 60.0), _lane(2.0 * 8 + 2.0, 62.5)]
    specs = [arterial(300.0, 300.0), arterial(2.0 * 3 + 2.0 + 0.775 + 0.095, 2.1 + 0.095, dims=BIKE_DIMS), arterial(20.0, -4.6)]
    out.append(dict(label="3 scripted vehicles, one a cyclist, a group of 4", paths=paths, sizes=[4], specs=specs, w=20, hit_o={0: 3, 2: 5}, near={0: 1}))
    for g in out:
        g["x0"] = np.array([[p[0, 0], p[0, 1], 0.0, p[0, 2]] for p in g["paths"]])
        g["shapes"] = [SN.shape_of(**{"L": s["dims"]["L"], "width": s["dims"]["width"], "extra_length": s["dims"]["extra_length"]})
                       if s.get("dims") else CAR for s in g["specs"]]
    return out


def group_ego_cases(g):
    """The egos of a group case as cases: the scripted vehicles' get() tuples, then the mates (x, y, v, yaw, 0, 0) in batch order."""
    B = len(g["paths"])
    scripted = [(s["x_init"], s["y_init"], s["speed"], UP, 0.0, 0.0) for s in g["specs"]]
    mates = [(x, y, v, yaw, 0.0, 0.0) for x, y, v, yaw in g["x0"]]
    return [case(f"{g['label']}: ego {e}", g["paths"][e], 0.0, scripted + [mates[m] for m in range(B) if m != e],
                 g["shapes"] + [CAR] * (B - 1), w=g["w"], idx=0, prev=-1, ref=False) for e in range(B)]
