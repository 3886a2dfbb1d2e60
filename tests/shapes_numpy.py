"""numpy restatement of the loop glue with one shape PER OBSTACLE (jsim_loop_set_vehicle_shapes): oracle/loop_oracle.py's
first_collision / first_collision_fast / loop_pre_tick with per-obstacle circle offsets, wheelbase and min_distance = ego
radius + the obstacle's own radius (check_collision_moving_bicycle's, main/lib/collision_avoidance.py:137).  TEST
INFRASTRUCTURE ONLY.

The oracle takes one obst_dims for all obstacles; with every obstacle of one shape this module equals it exactly
(tests/test_vehicle_shapes_cpu.py pins that on the reference-made cases of loop_f1.npz and loop_bicycle.npz).  The mixed case
has no reference function behind it -- the reference never mixes shapes: it is the same row order (frame, ego circle, obstacle
in list order, frame offset, obstacle circle) and first-hit rule with each obstacle's own numbers.

A shape is (cc_front, cc_rear, radius, wheelbase), the row of the C-ABI's table."""
import math

import numpy as np

import loop_oracle as LO

CAR = (2.86, 2.0, 0.64)      # BicycleModelDimensions of the egos (lib/car_dimensions.py:62-79)
BIKE = (1.0, 0.45, 0.64)     # BicycleRealDimensions (lib/car_dimensions.py:92-100)


def shape_of(L=2.86, width=2.0, extra_length=0.64):
    radius, (c0, c1) = LO.car_circles(L, width, extra_length)
    return (c0, c1, radius, L)


def _ego(L):
    radius, offs = LO.car_circles(L)
    return radius, offs


def first_collision(res, detailed, preds, shapes, L=2.86, frame_window=LO.FRAME_WINDOW):
    """The plain nested-loop form, written like loop_oracle.first_collision.  Returns (x, y, first, obstacle) or None."""
    if len(preds) == 0:
        return None
    radius, offs = _ego(L)
    P = len(preds[0])
    F = max(len(res), max(len(p) for p in preds))
    ego_cc = [LO.circle_centres(res, xo) for xo in offs]
    obs_cc = [[LO.circle_centres(p, xo) for xo in sh[:2]] for p, sh in zip(preds, shapes)]
    hit = None
    for f in range(F):
        fa = min(f, len(res) - 1)
        fo = min(f, P - 1)
        for a in range(2):
            pa = ego_cc[a][fa]
            for o in range(len(preds)):
                thr = radius + shapes[o][2]
                for off in range(-frame_window, frame_window + 1):
                    j = min(max(fo - off, 0), P - 1)
                    for b in range(2):
                        po = obs_cc[o][b][j]
                        dx, dy = pa[0] - po[0], pa[1] - po[1]
                        if math.sqrt(dx * dx + dy * dy) <= thr:
                            hit = (po, o)
                            break
                    if hit is not None:
                        break
                if hit is not None:
                    break
            if hit is not None:
                break
        if hit is not None:
            break
    if hit is None:
        return None
    po, o = hit
    thr = radius + shapes[o][2]
    first = 0
    for a in range(2):
        cc = LO.circle_centres(detailed, offs[a])
        dx, dy = po[0] - cc[:, 0], po[1] - cc[:, 1]
        m = np.sqrt(dx * dx + dy * dy) <= thr
        if m.any():
            first = int(np.argmax(m))
            break
    return float(detailed[first, 0]), float(detailed[first, 1]), first, o


def first_collision_fast(res, detailed, preds, shapes, L=2.86, frame_window=LO.FRAME_WINDOW):
    """Vectorised form (same row order).  Returns (x, y, first, obstacle) or None."""
    if len(preds) == 0:
        return None
    radius, offs = _ego(L)
    P = len(preds[0])
    F = max(len(res), max(len(p) for p in preds))
    w = frame_window
    fa = np.minimum(np.arange(F), len(res) - 1)
    fo = np.minimum(np.arange(F), P - 1)
    offv = np.arange(-w, w + 1)
    j = np.clip(fo[:, None] - offv[None, :], 0, P - 1)                       # [F, 2w+1]
    ego = np.stack([LO.circle_centres(res, xo)[fa] for xo in offs], axis=1)   # [F, a, 2]
    obs = np.stack([np.stack([LO.circle_centres(p, xo)[j] for xo in sh[:2]], axis=2) for p, sh in zip(preds, shapes)],
                   axis=1)                                                    # [F, o, off, b, 2]
    thr = np.array([radius + sh[2] for sh in shapes])                         # [o]
    d = ego[:, :, None, None, None, :] - obs[:, None, :, :, :, :]             # [F, a, o, off, b, 2]
    m = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) <= thr[None, None, :, None, None]
    flat = m.reshape(-1)
    k = int(np.argmax(flat))
    if not flat[k]:
        return None
    f, a, o, io, b = np.unravel_index(k, m.shape)
    hit = obs[f, o, io, b]
    n = len(detailed)
    cc = np.concatenate([LO.circle_centres(detailed, xo) for xo in offs])
    dx, dy = hit[0] - cc[:, 0], hit[1] - cc[:, 1]
    mm = np.sqrt(dx * dx + dy * dy) <= thr[o]
    first = int(np.argmax(mm)) % n
    return float(detailed[first, 0]), float(detailed[first, 1]), first, int(o)


def predict(obstacles, shapes, dt=LO.DT):
    """Every obstacle's prediction with its own wheelbase."""
    return [LO.predict_obstacle(*o, dt=dt, L=sh[3]) for o, sh in zip(obstacles, shapes)]


def loop_pre_tick(state_xyyawv, traj_agent_idx, prev_path_len, full, obstacles, dl, shapes, L=2.86, dt=LO.DT, margin_factor=4,
                  frame_window=LO.FRAME_WINDOW, preds=None):
    """loop_oracle.loop_pre_tick with per-obstacle shapes: (status, traj_agent_idx, path_len, collision_xy or None, first index
    on the detailed path or -1, index of the obstacle hit or -1).  preds: predictions made elsewhere (else from `obstacles`)."""
    import oracle_py as O
    x, y, yaw, v = state_xyyawv
    M = len(full)
    if prev_path_len is None or traj_agent_idx != prev_path_len - 1:
        st, idx = O.nearest_index_in_direction(x, y, full[:, 0], full[:, 1], traj_agent_idx, True)
        if st != 0:
            return st, traj_agent_idx, prev_path_len if prev_path_len is not None else M, None, -1, -1
        traj_agent_idx = idx
    detailed = full[traj_agent_idx:]
    res = detailed[LO.resample_mask(detailed[:, :2], LO.ego_resample_dl(len(detailed), v, dt))]
    if preds is None:
        preds = predict(obstacles, shapes, dt)
    col = first_collision_fast(res, detailed, preds, shapes, L=L, frame_window=frame_window)
    if col is None:
        return 0, traj_agent_idx, M, None, -1, -1
    c = LO.cutoff_index(full, col[0], col[1])
    assert c is not None
    cut = max(traj_agent_idx + 1, c - (LO.extra_cutoff_margin(dl, L) // 4) * margin_factor)
    return 0, traj_agent_idx, cut, (col[0], col[1]), col[2], col[3]
