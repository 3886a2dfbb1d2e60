"""Checkpoints of a running loop on the device (checkpoint_every=, restore, fork(warm=True), save_checkpoints / load_checkpoints;
jsim_loop_checkpoint_save / _load).  The feature copies state, so every comparison is torch.equal /
np.array_equal: a run with checkpoints against the run without; the slots against clones of the live state; a rewound run against
the run it rewinds, in both glue modes; a warm fork against the source's later ticks, where a cold fork differs; a counterfactual
against a loop built by hand; interacting groups under both mate predictions; the other kernels, a dense window, another process,
and the refusals."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import checkpoint_cases as CC
import checkpoint_numpy as CN
from checkpoint_cases import AGE, B, EVERY, GOAL, N, T
from conftest import REPO
from gpu_helpers import W, iroutes, loop_engine, loop_state, obstacle_state, sub_batch  # noqa: F401

pytestmark = pytest.mark.gpu

# every live tensor of a glue loop's state, named as history.CHECKPOINT names its slab -- the test's own list
LIVE = dict(x0=lambda l: l.loop.x0, x0_spawn=lambda l: l.loop.x0_spawn, target_spawn=lambda l: l.loop.target_spawn, age=lambda l: l.loop.age,
            tick_counter=lambda l: l.loop.tick_counter, n_respawn=lambda l: l.loop.n_respawn, target_ind=lambda l: l.loop.eng.target_ind,
            oa=lambda l: l.loop.eng.oa, od=lambda l: l.loop.eng.od, di_ai=lambda l: l.loop.eng.di_ai, status=lambda l: l.loop.eng.status,
            path_len=lambda l: l.loop.eng.path_len, cv_cut=lambda l: l.loop.eng.cv_cut, traj_idx=lambda l: l.pre.traj_idx,
            prev_len=lambda l: l.pre.prev_len, col_flag=lambda l: l.pre.col_flag, pre_status=lambda l: l.pre.status,
            obs_state=lambda l: l.obst.state)


def same(a, b):
    """torch.equal with NaN equal to NaN (a failed solve records no xref deviation)."""
    return torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)) if a.is_floating_point() else torch.equal(a, b)


def clones(loop):
    return {k: f(loop).clone() for k, f in LIVE.items() if f(loop) is not None}


def records(loop, k0=0, k1=None):
    """Clones of what the recorder holds of ticks [k0, k1): rec, flags, the vehicles' tuples and the plans."""
    r = loop.recorder
    d = dict(rec=r.rec[k0:k1], flags=r.flags[k0:k1])
    if r.obs is not None:
        d["obs"] = r.obs[k0:k1]
    if r.plans is not None:
        d.update({k: v[k0:k1] for k, v in r.plans.items()})
    return {k: v.clone() for k, v in d.items()}


def assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        assert same(a[k], b[k]), (what, k)


def during(loop):
    """The loop's written slots of ticks before N (save_checkpoints adds the one of the tick the loop stands at)."""
    return [c for c in loop.checkpoints if c[1] < N]


def mid_episode(flags, k):
    """The egos for which tick k lies within an episode that began before it ([B] bool), from the flags [n][B]."""
    return ((flags[k - 1] & (GOAL | AGE)) == 0).cpu().numpy()


@pytest.fixture(scope="module")
def base(pkg, iroutes):
    """The base loop after run(N) with checkpoint_every = EVERY: the source of the forks; nothing below changes it."""
    loop = CC.scenario_loop(pkg, iroutes, checkpoint_every=EVERY)
    loop.run(N)
    return loop


@pytest.fixture(scope="module")
def ticked(pkg, iroutes):
    """The same loop driven by N host tick()s, with clones of every state tensor ahead of the checkpoint ticks."""
    loop = CC.scenario_loop(pkg, iroutes, checkpoint_every=EVERY)
    live = {}
    for k in range(N):
        if k % EVERY == 0:
            live[k] = clones(loop)
        loop.tick()
    return loop, live


# ---- 1. a run with checkpoints is the run without ----
def test_unchanged_run(pkg, iroutes, base):
    plain = CC.scenario_loop(pkg, iroutes)
    plain.run(N)
    assert plain.checkpoints == [] and plain.checkpoint_every is None
    assert during(base) == [(s, s * EVERY) for s in range(N // EVERY)] and base.checkpoint_every == EVERY
    a, b = loop_state(base), loop_state(plain)
    assert a.keys() == b.keys() and {"rec", "rec_flags", "x0", "oa", "col_flag", "pre_status", "path_len"} <= a.keys()
    assert_same(a, b, "loop state")
    assert_same(obstacle_state(base), obstacle_state(plain), "vehicles")
    assert_same(clones(base), clones(plain), "state")
    assert int(base.loop.tick_counter.item()) == N and int(base.loop.n_respawn.item()) >= B
    assert base.recorder.ticks_run == N and not base.recorder.overflow


# ---- 2. the slots are the live state ----
def test_slots_are_the_live_state(pkg, base, ticked):
    loop, live = ticked
    assert sorted(live) == [0, 25, 50, 75] and loop.checkpoints == [(s, s * EVERY) for s in range(4)]
    names = [a.name for a in pkg.history.CHECKPOINT]
    assert set(loop._ck.slabs) == set(names) - {"cv_cut"} == set(live[0])             # (the truncate glue has no speed cut-off)
    for s in range(4):
        for k, want in live[s * EVERY].items():
            assert torch.equal(loop._ck.slabs[k][s], want), (s, k)
            assert torch.equal(base._ck.slabs[k][s], want), ("the fused run", s, k)
    assert int(loop._ck.slabs["tick_counter"][2].item()) == 50
    mid = mid_episode(loop.recorder.flags, 50)
    warm = (loop._ck.slabs["oa"][2] != 0).any(dim=1).cpu().numpy()                    # a warm start there is to continue
    print(f"mid-episode at tick 50: egos {np.flatnonzero(mid).tolist()}, with a warm start {np.flatnonzero(warm).tolist()}")
    assert mid.sum() >= 4 and warm.sum() >= 4


# ---- 3. rewind ----
@pytest.mark.parametrize("mode", ("truncate", "speed_cutoff"))
def test_rewind(pkg, iroutes, mode):
    loop = CC.scenario_loop(pkg, iroutes, mode=mode, checkpoint_every=EVERY)
    loop.run(N)
    keep, end = records(loop, 0, N), clones(loop)
    assert ("cv_cut" in loop._ck.slabs) == (mode == "speed_cutoff")
    mid = mid_episode(loop.recorder.flags, 50)
    print(f"{mode}: mid-episode at tick 50: egos {np.flatnonzero(mid).tolist()}, respawns {int(loop.loop.n_respawn.item())}")
    assert mid.sum() >= 4                                                             # else the test proves no more than the cold fork does
    loop.restore(2)
    assert int(loop.loop.tick_counter.item()) == 50 and loop.checkpoints == [(0, 0), (1, 25), (2, 50)]
    loop.recorder.rec[50:].fill_(-1.0)                                                # the ticks that follow are written again
    loop.recorder.flags[50:].fill_(-1)
    loop.recorder.obs[50:].fill_(-1.0)
    loop.run(50)
    assert_same(records(loop, 0, N), keep, mode)
    assert_same(clones(loop), end, mode)
    assert loop.checkpoints == [(s, s * EVERY) for s in range(4)] and loop.recorder.ticks_run == N


# ---- 4. a warm fork continues; a cold one does not ----
def rows_equal_source(fork, src, ego, at, m):
    """Row r of the fork's first m records is ego ego[r] of the source from tick at[r] on, its set's vehicles included."""
    for r, (e, k) in enumerate(zip(ego, at)):
        assert same(fork.recorder.rec[:m, r], src.recorder.rec[k:k + m, e]), (r, e, k)
        assert torch.equal(fork.recorder.flags[:m, r], src.recorder.flags[k:k + m, e]), (r, e, k)
        s, s0 = int(fork.traffic[0][r]), int(src.traffic[0][e])
        lo, hi, lo0, hi0 = int(fork.traffic[1][s]), int(fork.traffic[1][s + 1]), int(src.traffic[1][s0]), int(src.traffic[1][s0 + 1])
        assert torch.equal(fork.recorder.obs[:m, lo:hi], src.recorder.obs[k:k + m, lo0:hi0]), (r, e, k)


def assert_loaded(pkg, fork, src, ego, at):
    """The fork's live state is the restatement's gather (tests/checkpoint_numpy.py) of the source's slabs, its traffic sets the
    restatement's."""
    tick_slot = {t: s for s, t in src.checkpoints}
    tof, veh_src, veh_tick = CN.fork_traffic([int(src.traffic[0][e]) for e in ego], [int(k) for k in at], [int(v) for v in src.traffic[1]])
    want = CN.load({k: v.cpu().numpy() for k, v in src._ck.slabs.items()}, {a.name: a.per for a in pkg.history.CHECKPOINT},
                   [int(e) for e in ego], [tick_slot[int(k)] for k in at], veh_src, [tick_slot[k] for k in veh_tick])
    live = clones(fork)
    assert set(want) == set(live) - {"tick_counter", "n_respawn"} and fork.traffic[0].tolist() == tof
    for k, v in want.items():
        assert np.array_equal(live[k].cpu().numpy(), v), k
    assert int(fork.loop.tick_counter.item()) == 0 and int(fork.loop.n_respawn.item()) == 0


def test_warm_fork(pkg, base):
    ego, m = np.arange(B), 50
    keep = records(base, 0, N)
    fork = base.fork(ego, 50, warm=True, record=m)
    assert_loaded(pkg, fork, base, ego, [50] * B)
    assert fork.checkpoints == [] and torch.equal(fork.loop.x0, base._ck.slabs["x0"][2]) and int(fork.loop.tick_counter.item()) == 0
    assert torch.equal(fork.recorder.x0_first, fork.loop.x0) and torch.equal(fork.obst._state0, fork.obst.state)
    fork.run(m)
    rows_equal_source(fork, base, ego, [50] * B, m)
    # the same rows forked cold start every controller again: they differ wherever the tick lay within an episode
    mid = mid_episode(base.recorder.flags, 50)
    cold = base.fork(ego, 50, record=m)
    cold.run(m)
    differs = np.array([not same(cold.recorder.rec[:m, r], base.recorder.rec[50:N, r]) for r in range(B)])
    print(f"mid-episode egos {np.flatnonzero(mid).tolist()}, the cold fork differs on {np.flatnonzero(differs).tolist()}")
    assert mid.sum() >= 4 and differs[mid].all()
    # rows at ticks of their own in one fork, one ego twice
    ego2, at2 = np.array([0, 1, 2, 3, 1, 5]), np.array([25, 75, 25, 75, 25, 75])
    two = base.fork(ego2, at2, warm=True, record=25)
    assert_loaded(pkg, two, base, ego2, at2)
    two.run(25)
    rows_equal_source(two, base, ego2, at2, 25)
    assert_same(records(base, 0, N), keep, "the source is left as it was")
    assert not base.recorder.superseded and during(base) == [(s, s * EVERY) for s in range(4)]


# ---- 5. a counterfactual equals a loop built by hand ----
def test_counterfactual(pkg, iroutes, ticked):
    src, live = ticked
    eng, m = src.loop.eng, 50
    cfgs = [dataclasses.replace(eng.config, w_para=eng.config.w_para * (1.5 + 0.1 * b)) for b in range(B)]
    speed = eng.speed.cpu().numpy() * 0.8
    fork = src.fork(np.arange(B), 50, warm=True, record=m, ego_configs=cfgs, speed=speed)
    fork.run(m)
    # by hand, on a new engine, from the clones of tick 50: load_state and plain copies
    st = live[50]
    e2 = pkg.BatchedMPC([p.copy() for p in eng.paths], eng.path_id.cpu().numpy(), dl=eng.dl, T=T, speed=speed, config=eng.config, smooth=False)
    e2.set_ego_configs(cfgs)
    hand = pkg.ScenarioLoop(e2, st["x0"].clone(), CC.SETS, max_age=CC.MAX_AGE, frame_window=20, traffic_of=CC.TRAFFIC_OF, record=m)
    e2.load_state(st["target_ind"], st["oa"], st["od"])
    for dst, k in ((hand.loop.x0_spawn, "x0_spawn"), (hand.loop.target_spawn, "target_spawn"), (hand.loop.age, "age"), (e2.di_ai, "di_ai"),
                   (e2.status, "status"), (e2.path_len, "path_len"), (hand.pre.traj_idx, "traj_idx"), (hand.pre.prev_len, "prev_len"),
                   (hand.pre.col_flag, "col_flag"), (hand.pre.status, "pre_status"), (hand.obst.state, "obs_state")):
        dst.copy_(st[k])
    hand.run(m)
    assert_same(records(fork, 0, m), records(hand, 0, m), "counterfactual")
    assert_same(loop_state(fork), loop_state(hand), "counterfactual: loop state")
    assert_same(obstacle_state(fork), obstacle_state(hand), "counterfactual: vehicles")
    assert not same(fork.recorder.rec[:m], src.recorder.rec[50:N])                     # (it is another run than the source's)
    assert torch.equal(fork.recorder.obs[:m], src.recorder.obs[50:N])                  # .. beside the same vehicles


# ---- 6. interacting groups ----
VEHICLE = dict(direction=1, turning=True, speed=20 / 3.6, offset=2.0)
OTHER = {"plan": "constant", "constant": "plan"}


def interacting(pkg, W, iroutes, mode, **kw):
    """Two groups of three and two egos beside one scripted vehicle."""
    batch8, _ = W.interacting_batch(iroutes, 2, T, seed=0)
    eng, x0 = loop_engine(pkg, iroutes, sub_batch(batch8, np.array([0, 1, 2, 4, 5])), T)
    return pkg.InteractingLoop(eng, x0, group_sizes=[3, 2], obstacle_specs=[VEHICLE], max_age=CC.MAX_AGE, mate_prediction=mode, **kw)


@pytest.mark.parametrize("mode", ("plan", "constant"))
def test_interacting(pkg, W, iroutes, mode):
    n, every, at, m = 60, 20, 40, 20
    src = interacting(pkg, W, iroutes, mode, record=n, record_plans=True, checkpoint_every=every)
    src.run(n)
    assert src.checkpoints == [(0, 0), (1, 20), (2, 40)]
    plain = interacting(pkg, W, iroutes, mode, record=n, record_plans=True)
    plain.run(n)
    assert_same(records(src, 0, n), records(plain, 0, n), "unchanged run")
    want = records(src, at, n)
    both = src.fork([0, 1], at, warm=True, record=m)
    assert both.mate_prediction == mode and both.group_off.tolist() == [0, 3, 5] and both.recorder.plans is not None
    both.run(m)
    assert_same(records(both, 0, m), want, "both groups")
    # one group alone: groups do not affect each other
    one = src.fork(1, at, warm=True, record=m)
    assert one.loop.eng.B == 2 and one.group_off.tolist() == [0, 2]
    one.run(m)
    assert_same(records(one, 0, m), {k: (v if k == "obs" else v[:, 3:5]) for k, v in want.items()}, "group 1 alone")
    # the same group under the other mate prediction: a run of its own
    other = src.fork(0, at, warm=True, record=m, mate_prediction=OTHER[mode])
    assert other.mate_prediction == OTHER[mode]
    other.run(m)
    assert other.recorder.ticks_run == m
    assert not same(other.recorder.rec[:m], want["rec"][:, 0:3])
    # the old refusal stays: without warm=True, and on a loop without checkpoints
    for loop, kw in ((src, {}), (plain, dict(warm=True))):
        with pytest.raises(ValueError, match="warm starts .* are not recorded"):
            loop.fork(0, 1, **kw)
    with pytest.raises(ValueError, match="tick 30 is not checkpointed .*20 and 40"):
        src.fork(0, 30, warm=True)
    with pytest.raises(ValueError, match=r"ego 2 outside \[0, 2\)"):
        src.fork(2, 40, warm=True)


# ---- 7. the other kernels, a dense window, another process, refusals ----
def test_closed_loop_rewind(pkg, W, iroutes):
    eng, x0 = loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, T, rank=3), T)
    loop = pkg.ClosedLoop(eng, x0, max_age=CC.MAX_AGE, record=60, checkpoint_every=20)
    assert set(loop._ck.slabs) == {"x0", "x0_spawn", "target_spawn", "age", "tick_counter", "n_respawn", "target_ind", "oa", "od", "di_ai",
                                   "status", "path_len"}
    loop.run(30)
    for _ in range(30):
        loop.tick()                                                                   # (host ticks save too)
    assert loop.checkpoints == [(0, 0), (1, 20), (2, 40)]
    keep = records(loop, 0, 60)
    loop.restore(1)
    loop.recorder.rec[20:].fill_(-1.0)
    loop.run(40)
    assert_same(records(loop, 0, 60), keep, "ClosedLoop")
    assert int(loop.tick_counter.item()) == 60 and loop.checkpoints == [(0, 0), (1, 20), (2, 40)]
    with pytest.raises(ValueError, match="cannot be captured"):
        loop.capture(2)


@pytest.mark.parametrize("horizon, egos", ((14, 6), (40, 2)))
def test_rewind_on_the_other_kernels(pkg, iroutes, horizon, egos):
    """The LDS kernel (T = 14 has no register kernel: host-driven ticks) and a four-wave horizon."""
    loop = CC.scenario_loop(pkg, iroutes, T=horizon, B=egos, record=40, checkpoint_every=10)
    loop.run(40)
    keep, end = records(loop, 0, 40), clones(loop)
    loop.restore(2)
    loop.recorder.rec[20:].fill_(-1.0)
    loop.run(20)
    assert_same(records(loop, 0, 40), keep, horizon)
    assert_same(clones(loop), end, horizon)


def test_dense_window_and_a_fork_at_an_odd_tick(pkg, iroutes, base):
    with pytest.raises(ValueError, match=r"needs 101 slots, the loop has 5 \(construct it with checkpoint_slots=101\)"):
        base.checkpoint_every = 1
    assert base.checkpoint_every == EVERY
    loop = CC.scenario_loop(pkg, iroutes, checkpoint_every=EVERY, checkpoint_slots=N + 1)
    loop.run(N)
    keep = records(loop, 0, N)
    loop.restore(2)
    loop.checkpoint_every = 1
    loop.run(10)
    assert loop.checkpoints == [(0, 0), (1, 25), (2, 50)] + [(k, k) for k in range(50, 60)]
    assert_same(records(loop, 0, N), keep, "the window run again")
    at, m = 53, 30
    fork = loop.fork(np.arange(B), at, warm=True, record=m)
    fork.run(m)
    rows_equal_source(fork, loop, np.arange(B), [at] * B, m)
    with pytest.raises(ValueError, match=r"tick 60 is not checkpointed \(the nearest checkpointed ticks: 59\)"):
        loop.fork(0, 60, warm=True)                                                   # (the tick the loop stands at: saved by what follows)
    with pytest.raises(ValueError, match=r"tick 61 outside \[0, 60\]"):
        loop.fork(0, 61, warm=True)


def test_continue_from_the_file_in_a_fresh_process(pkg, base, tmp_path):
    path, out = str(tmp_path / "ck.npz"), str(tmp_path / "out.npz")
    base.save_checkpoints(path)
    assert base.checkpoints == [(s, s * EVERY) for s in range(5)]                      # (the state the loop stands at is saved first)
    assert torch.equal(base._ck.slabs["x0"][4], base.loop.x0)
    slabs, meta = pkg.history.read_checkpoint_file(path)
    assert meta["kind"] == "ScenarioLoop" and meta["slot_tick"].tolist() == [0, 25, 50, 75, 100] and meta["every"] == EVERY
    for k, v in slabs.items():
        assert np.array_equal(v, base._ck.slabs[k].cpu().numpy()), k
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([REPO] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "checkpoint_child.py"), path, "3", "25", out], env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = np.load(out)
    r = base.recorder
    assert int(got["k0"]) == 75 and int(got["ticks_run"]) == N
    nan = lambda a: np.nan_to_num(a, nan=-7.0)                                         # noqa: E731
    assert np.array_equal(nan(got["rec"]), nan(r.rec[75:N].cpu().numpy())) and np.array_equal(got["flags"], r.flags[75:N].cpu().numpy())
    assert np.array_equal(got["obs"], r.obs[75:N].cpu().numpy()) and np.array_equal(got["x0"], base.loop.x0.cpu().numpy())


def test_refusals(pkg, W, iroutes, base, tmp_path):
    eng = base.loop.eng
    for slot in (5, -1, 7, 1.0, True):
        with pytest.raises(ValueError, match="holds no checkpoint"):
            base.restore(slot)
    plain = CC.scenario_loop(pkg, iroutes, record=8)
    for call in (lambda: plain.restore(0), lambda: plain.fork(0, 0, warm=True), lambda: plain.save_checkpoints(str(tmp_path / "x.npz")),
                 lambda: setattr(plain, "checkpoint_every", 2)):
        with pytest.raises(ValueError, match="keeps no checkpoints"):
            call()
    with pytest.raises(ValueError, match=r"row 1: tick 30 is not checkpointed \(the nearest checkpointed ticks: 25 and 50\)"):
        base.fork([0, 1], [25, 30], warm=True)
    with pytest.raises(ValueError, match=r"ego 6 outside \[0, 6\)"):
        base.fork(6, 25, warm=True)
    with pytest.raises(ValueError, match="at least one row"):
        base.fork([], [], warm=True)
    for kw in (dict(paths=[iroutes[0].copy()], path_id=0), dict(path_id=0), dict(cv=[np.ones(3)])):
        with pytest.raises(ValueError, match="a warm start belongs to its path"):
            base.fork(0, 25, warm=True, **kw)
    with pytest.raises(ValueError, match="holds fewer than the 5 slots"):
        CC.scenario_loop(pkg, iroutes, checkpoint_every=EVERY, checkpoint_slots=4)
    # a file of another loop
    cl = pkg.ClosedLoop(*loop_engine(pkg, iroutes, W.ego_batch(iroutes, B, T, rank=3), T), record=N, checkpoint_every=EVERY)
    path = str(tmp_path / "ck.npz")
    base.save_checkpoints(path)
    with pytest.raises(ValueError, match="holds the checkpoints of a ScenarioLoop, this loop is a ClosedLoop"):
        cl.load_checkpoints(path)
    with pytest.raises(ValueError, match="cannot be captured"):
        cl.capture(2)
    # the C calls with a context: refused before any device call, the message on the context
    lib, ctx = eng.lib, eng._ctx
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)                                   # noqa: E731
    x0, slab = base.loop.x0, base._ck.slabs["x0"]
    before = x0.clone()
    src, dst = np.array([slab.data_ptr()], dtype=np.uint64), np.array([x0.data_ptr()], dtype=np.uint64)
    for nbytes, msg in ((-8, "array 0: bytes=-8"), (6, "array 0: bytes=6")):
        assert lib.jsim_loop_checkpoint_save(ctx, 1, vp(src), vp(dst), vp(np.array([nbytes], dtype=np.int64)), None) == -22
        assert msg in lib.jsim_last_error(ctx).decode()
    assert lib.jsim_loop_checkpoint_save(ctx, 33, vp(src), vp(dst), vp(np.array([8], dtype=np.int64)), None) == -22
    i32 = lambda *v: np.array(v, dtype=np.int32)                                       # noqa: E731
    written, row_bytes = i32(1, 1, 0, 1, 1), np.array([32], dtype=np.int64)
    for ego, slot, msg in ((i32(0, 6), i32(0, 1), "row 1: ego=6 outside [0, B=6)"), (i32(0, 1), i32(0, 2), "row 1: slot=2 is not a written slot"),
                           (i32(0, 1), i32(5, 0), "row 0: slot=5 is not a written slot")):
        rc = lib.jsim_loop_checkpoint_load(ctx, B, 5, vp(written), 2, vp(ego), vp(slot), 1, vp(src), vp(dst), vp(row_bytes), 0, None, 0, None, None,
                                           None, None)
        assert rc == -22 and msg in lib.jsim_last_error(ctx).decode(), msg
    torch.cuda.synchronize()
    assert torch.equal(x0, before)
