"""Shared pieces of the GPU parity tests (tests/test_gpu_*.py)."""
import dataclasses
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG_NAME

_CONFIG = importlib.import_module(PKG_NAME + ".config")
REG_VARIANTS = _CONFIG.REG_VARIANTS
_CABI = importlib.import_module(PKG_NAME + "._cabi")
W2_MIN_B = 1025          # launch_reg's JSIM_W2_MIN_B default (csrc/reg_variants.h); the tests never set it, nor JSIM_HELP_MAX_B


def variant_id(row):
    """A readable test id for a row (W, T, PRE, WPE, HELP) of config.REG_VARIANTS: w1-T15-pre-wpe1, w1-T20-wpe1-help."""
    W, T, pre, wpe, help_ = row
    return f"w{W}-T{T}" + ("-pre" if pre else "") + f"-wpe{wpe}" + ("-help" if help_ else "")


def variant_batches(row, cu):
    """The batch sizes at which launch_reg takes `row` (select_reg_variant with JSIM_HELP_MAX_B = cu, the device's CU count, and
    JSIM_W2_MIN_B = 1025), each at a boundary where the dispatch changes: HELP rows at B = cu, the last size with one ego per CU;
    one-wave rows without helpers at cu + 1, the first size without them, and below the two-waves-per-SIMD threshold at 1024 where
    that horizon has a two-wave form; that form at cu + 1 where it is the horizon's only one-wave form, else at 1025; the four-wave
    rows at an odd size.  tests/test_host_cpu.py checks the dispatch lands on every row at every size returned here."""
    W, T, pre, wpe, help_ = row
    w1 = (1, T, pre, 1, False) in REG_VARIANTS
    if help_:
        return (cu,)
    if W == 1 and wpe == 2:
        return (W2_MIN_B,) if w1 else (cu + 1,)
    if W == 1:
        return (cu + 1, W2_MIN_B - 1) if (1, T, pre, 2, False) in REG_VARIANTS else (cu + 1,)
    return (97,)


def variant_batch(row, cu):
    """The first of variant_batches(row, cu)."""
    return variant_batches(row, cu)[0]


def cu_count():
    """The CU count of device 0: launch_reg's HELP threshold."""
    return torch.cuda.get_device_properties(0).multi_processor_count


def iter_totals(eng, reset=False):
    """jsim_mpc_iter_totals of an engine's context: the per-ego active-set iterations of its closed-loop runs (int64 [B])."""
    tot = np.zeros(eng.B, dtype=np.uint64)
    _CABI.check(eng.lib.jsim_mpc_iter_totals(eng._ctx, eng.B, tot.ctypes.data, 1 if reset else 0), eng._ctx, "jsim_mpc_iter_totals")
    return tot.astype(np.int64)


# ------------------------------------------------------------------------------------------------
# The closed loops (ClosedLoop / ScenarioLoop / InteractingLoop): workload fixtures, engines, and snapshots of everything a loop
# leaves on the device.  A test module takes the fixtures by importing them.
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def W(pkg):
    return importlib.import_module(PKG_NAME + ".workloads")


@pytest.fixture(scope="module")
def iroutes(W):
    return W.route_table(False)[0]


def sub_batch(batch, idx):
    """The egos idx of an EgoBatch."""
    return dataclasses.replace(batch, **{f.name: getattr(batch, f.name)[idx] for f in dataclasses.fields(batch)})


def loop_engine(pkg, routes, batch, T, mode="truncate"):
    """(engine, x0) for a loop of glue `mode` on device 0: workloads.make_engine."""
    return pkg.workloads.make_engine(routes, batch, T, "cuda:0", mode=mode)


def loop_state(loop, idx=None, exclude=()):
    """Clones of every per-ego buffer of a ScenarioLoop / InteractingLoop (rows idx): loop, glue and engine buffers, the predicted
    states, the speed cut-off when the glue has one, the history, and the recorder's records when one is attached."""
    eng, cl, pre = loop.loop.eng, loop.loop, loop.pre
    d = dict(x0=cl.x0, path_len=eng.path_len, target_ind=eng.target_ind, traj_idx=pre.traj_idx, prev_len=pre.prev_len,
             col_flag=pre.col_flag, pre_status=pre.status, status=eng.status, oa=eng.oa, od=eng.od, di_ai=eng.di_ai, age=cl.age,
             ox=eng.ox, oy=eng.oy, ov=eng.ov, oyaw=eng.oyaw)
    if pre.cut is not None:
        d["cut"] = pre.cut
    if idx is not None:
        d = {k: v.index_select(0, idx) for k, v in d.items()}
    by_tick = dict(hist=cl.hist)                                  # [ticks, B, ...]
    if loop.recorder is not None:
        by_tick.update(rec=loop.recorder.rec, rec_flags=loop.recorder.flags)
    d.update({k: v if idx is None else v.index_select(1, idx) for k, v in by_tick.items() if v is not None})
    return {k: v.clone() for k, v in d.items() if k not in exclude}


def obstacle_state(loop, lo=0, hi=None):
    """Clones of the scripted vehicles lo..hi of a loop: states, get() tuples, and the recorder's tuples when it keeps them."""
    hi = loop.obst.n if hi is None else hi
    d = dict(state=loop.obst.state[lo:hi], get=loop.obst.get_buf[lo:hi])
    if loop.recorder is not None and loop.recorder.obs is not None:
        d["rec_obs"] = loop.recorder.obs[:, lo:hi]
    return {k: v.clone() for k, v in d.items()}


def assert_state_equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------------------------------------
# The guarded launch of the recorder's evaluators (jsim_loop_eval_*): outputs poisoned first, one row of guard slots in front of the
# [n][B] the call may write and one behind.
# ------------------------------------------------------------------------------------------------
def guarded_outputs(spec, n, B, dev):
    """(views, buffers) of the outputs `spec` -- (key, numpy dtype, trailing shape, poison: a value the output cannot take) each --:
    buffers [n + 2][B]... filled with the poison, and their rows from 1 on -- the [n][B]... the call may write, whose pointers it
    takes, and the guard row behind (so that n = 0 still has a pointer)."""
    buf = {k: torch.full((n + 2, B) + tuple(shape), poison, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, dt, shape, poison in spec}
    return {k: b[1:] for k, b in buf.items()}, buf


def check_guarded(pkg, eng, name, spec, buf, n, rc, rc_want=0, nothing=False, what=()):
    """Behind a call of entry point `name` on guarded_outputs' views that returned rc.  rc_want != 0 (a refusal) or `nothing` (n = 0
    or B = 0): rc is the wanted one and every slot is still poison; returns the library's last message.  Else the call succeeded,
    the guards are intact and no slot between is poison; returns the rows [1, n + 1) as numpy arrays."""
    torch.cuda.synchronize()
    poison = {k: p for k, _, _, p in spec}
    host = {k: v.cpu().numpy() for k, v in buf.items()}
    if rc_want != 0 or nothing:                                            # refused, or nothing to do: nothing is written
        assert rc == rc_want, rc
        assert all(np.all(host[k] == poison[k]) for k in poison)
        return eng.lib.jsim_last_error(eng._ctx).decode()
    pkg._cabi.check(rc, eng._ctx, name)
    for k in poison:
        assert np.all(host[k][0] == poison[k]) and np.all(host[k][n + 1] == poison[k]), ("guard", k, *what, n)
        assert not np.any(host[k][1:n + 1] == poison[k]), ("unwritten", k, *what, n)
    return {k: host[k][1:n + 1] for k in poison}


def engine(pkg, routes, batch, T, **kw):
    eng = pkg.BatchedMPC(routes, batch.path_id, dl=pkg.synth.DL, T=T, speed=batch.speed, device="cuda:0", smooth=False, **kw)
    eng.load_state(batch.target_ind, batch.oa, batch.od, batch.path_len)
    return eng


def debug_bufs(eng, n=None):
    """The debug outputs of BatchedMPC.solve; with n (the QP's variables: 2T, 2T + 1 for the acceleration-state variant) only the
    condensed QP and its multipliers."""
    B, T = eng.B, eng.T
    f = dict(dtype=torch.float64, device=eng.device)
    if n is not None:
        return {"H": torch.zeros(B, n, n, **f), "g": torch.zeros(B, n, **f), "lam": torch.zeros(B, 8 * T, **f)}
    return {"xbar": torch.zeros(B, 4, T + 1, **f), "ref_idx": torch.zeros(B, T + 1, dtype=torch.int64, device=eng.device),
            "H": torch.zeros(B, 2 * T, 2 * T, **f), "g": torch.zeros(B, 2 * T, **f), "lam": torch.zeros(B, 8 * T, **f)}


def oracle_batch(oracle, pkg, routes, batch, T, n_threads=1, **kw):
    p = oracle.make_params(T=T, **kw)
    cx, cy, cyaw, off = pkg.synth.pack_paths(routes)
    return p, oracle.mpc_step_batch(p, batch.x0, batch.path_id, batch.path_len, batch.speed, cx, cy, cyaw, off,
                                    batch.target_ind, batch.oa, batch.od, n_threads=n_threads)


# ------------------------------------------------------------------------------------------------
# The per-ego table (BatchedMPC.set_ego_configs / jsim_mpc_set_ego_config): inputs shared by tests/test_gpu_ego_config.py and
# tests/test_ego_config_cpu.py, which proves on the oracle alone that these inputs keep the comparisons meaningful.
# ------------------------------------------------------------------------------------------------
EGO_CFG_SEED, EGO_BATCH_SEED = 17, 4                  # the draws of test_per_ego_weights_one_batch
# planted egos, next to each other so that a row read one off shows: two twins (same state, path and warm start, very different
# rows), an ego that fails (v0 > speed) whose row brakes with -3.7, a row with tight limits beside a loose one
PLANT_TWINS, PLANT_FAIL, PLANT_TIGHT, PLANT_LOOSE = (10, 11), 12, 13, 14
PLANT_EGOS = PLANT_TWINS + (PLANT_FAIL, PLANT_TIGHT, PLANT_LOOSE)
PLANT_DECEL = -3.7
ORACLE_KEYS = ("NX", "w_perp", "w_para", "R", "Rd", "Q_v_yaw", "Qf", "GOAL_DIS", "STOP_SPEED", "MAX_ITER", "MAX_DSTEER", "MAX_ACCEL",
               "MAX_DECEL", "JERK_WEIGHT")


def ego_config_pool(T, n=12, seed=EGO_CFG_SEED, base=None):
    """n distinct MPCConfigs of horizon T, drawn as test_per_ego_weights_one_batch draws them (same ranges); everything the table
    does not carry stays `base`'s (default: the stock JSON)."""
    from dataclasses import replace
    rng = np.random.default_rng(seed)
    base = base if base is not None else _CONFIG.MPCConfig.from_json()
    return [replace(base, T=T, w_perp=float(rng.uniform(5, 40)), w_para=float(rng.uniform(0.5, 3)),
                    R=[float(rng.uniform(0.005, 0.2)), float(rng.uniform(0.005, 0.05))],
                    Rd=[float(rng.uniform(0.005, 10)), float(rng.uniform(0.5, 10))],
                    Q_v_yaw=[float(rng.choice([0.0, 2.0])), float(rng.uniform(0.1, 1.0))],
                    Qf=[float(rng.uniform(0.5, 2)), float(rng.uniform(0.5, 2)), 0.0, float(rng.uniform(0.2, 1.0))],
                    MAX_DSTEER=float(rng.uniform(10, 60)), MAX_ACCEL=float(rng.uniform(0.5, 3)),
                    MAX_DECEL=float(-rng.uniform(3, 10))) for _ in range(n)]


def ego_config_table(pool, B, seed=EGO_CFG_SEED, plant=True):
    """(cfgs, which): ego b solves with cfgs[b], a seeded pick from `pool`; egos with equal which[b] share a configuration, so the
    oracle side can group them.  plant: the rows of PLANT_EGOS are replaced by the planted ones (which >= len(pool))."""
    from dataclasses import replace
    rng = np.random.default_rng(seed + 1000)
    which = rng.integers(0, len(pool), size=B).astype(np.int64)
    cfgs = [pool[k] for k in which]
    if plant:
        assert B > max(PLANT_EGOS)
        a, b = PLANT_TWINS
        planted = {a: replace(cfgs[a], MAX_ACCEL=0.5, w_perp=5.0), b: replace(cfgs[a], MAX_ACCEL=3.0, w_perp=40.0),
                   PLANT_FAIL: replace(cfgs[PLANT_FAIL], MAX_DECEL=PLANT_DECEL),
                   PLANT_TIGHT: replace(cfgs[PLANT_TIGHT], MAX_ACCEL=0.05, MAX_DSTEER=0.4),
                   PLANT_LOOSE: replace(cfgs[PLANT_LOOSE], MAX_ACCEL=3.0, MAX_DSTEER=60.0)}
        for k, (e, c) in enumerate(sorted(planted.items())):
            cfgs[e], which[e] = c, len(pool) + k
    return cfgs, which


def plant_ego_states(routes, batch):
    """The states that go with the planted rows, in place: the twins share one state, path and warm start -- slow, early on an
    untruncated path with an accelerating warm start, so that MAX_ACCEL binds; so do the tight and the loose ego, off their path and
    turned away from it, so that the steering limits matter too; PLANT_FAIL starts above its speed limit."""
    for (a, b), lat, dyaw in ((PLANT_TWINS, 0.0, 0.0), ((PLANT_TIGHT, PLANT_LOOSE), 0.3, 0.1)):
        r = routes[int(batch.path_id[a])]
        s = len(r) // 6
        batch.x0[a] = (r[s, 0] - lat * np.sin(r[s, 2]), r[s, 1] + lat * np.cos(r[s, 2]), 2.0, r[s, 2] + dyaw)
        batch.target_ind[a], batch.path_len[a] = max(s - 3, 0), len(r)
        batch.oa[a] = 1.0
        for name in ("x0", "path_id", "path_len", "target_ind", "speed", "oa", "od"):
            getattr(batch, name)[b] = getattr(batch, name)[a]
    batch.x0[PLANT_FAIL, 2] = 9.5                       # v0 > speed: the reference's failure path, as test_step_vs_oracle plants it
    return batch


def ego_config_case(synth, routes, T, B, base=None, plant=True, **batch_kw):
    """The inputs of one per-ego case, on the GPU and on the CPU alike: (batch, cfgs, which) from the draws of
    test_per_ego_weights_one_batch (config seed 17, batch seed 4, truncated paths, a fifth of the egos near their path's end)."""
    kw = dict(seed=EGO_BATCH_SEED, truncate=True, near_end_frac=0.2)
    kw.update(batch_kw)
    batch = synth.make_ego_batch(routes, B, T, **kw)
    cfgs, which = ego_config_table(ego_config_pool(T, base=base), B, plant=plant)
    if plant:
        plant_ego_states(routes, batch)
    return batch, cfgs, which


def ego_config_rows(cfgs, reserved=0.0):
    """The [B, 16] array of include/jsim_mpc.h for cfgs, slot 15 (`reserved`) set to `reserved`."""
    return np.array([[c.w_perp, c.w_para, c.R[0], c.R[1], c.Rd[0], c.Rd[1], c.Q_v_yaw[0], c.Q_v_yaw[1], c.Qf[0], c.Qf[1], c.Qf[2],
                      c.Qf[3], c.max_dsteer_rad, c.MAX_ACCEL, c.MAX_DECEL, reserved] for c in cfgs], dtype=np.float64)


def oracle_params(oracle, cfg, T=None):
    """oracle.make_params for an MPCConfig: every key the oracle takes from a configuration."""
    return oracle.make_params(T=cfg.T if T is None else T, config={k: getattr(cfg, k) for k in ORACLE_KEYS})


def oracle_params_list(oracle, cfgs, which):
    """One OrcParams per distinct configuration, indexed by `which` (gaps, if any, stay None)."""
    out = [None] * (int(np.max(which)) + 1)
    for b, k in enumerate(which):
        if out[k] is None:
            out[k] = oracle_params(oracle, cfgs[b])
    return out


def oracle_batch_per_config(oracle, synth, routes, batch, cfgs, which, n_threads=16, **kw):
    """(params_list, oracle.mpc_step_batch_per_config(..)) of a batch: every ego by the oracle with its own configuration."""
    ps = oracle_params_list(oracle, cfgs, which)
    cx, cy, cyaw, off = synth.pack_paths(routes)
    return ps, oracle.mpc_step_batch_per_config(ps, which, batch.x0, batch.path_id, batch.path_len, batch.speed, cx, cy, cyaw, off,
                                                batch.target_ind, batch.oa, batch.od, n_threads=n_threads, **kw)


def n_active(mask):
    """Active rows per ego of an active-mask array [B, MW] (uint32 words)."""
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), axis=1).sum(axis=1)


def qp_constraints(T, dt, v0, speed, cfgs, min_speed, max_steer, jerk=False):
    """(G [8T, 2T], h [B, 8T]) of the condensed QP's G u <= h in the canonical row order (include/jsim_mpc.h), u = (a_0, delta_0,
    a_1, ...): G rows from the structure, h from each ego's start speed v0[b], speed limit speed[b] and limits cfgs[b].  The two
    t = 0 speed rows are constants (zero rows of G).
    jerk: the acceleration-state variant (main/lib/mpc_jerk.py), u = (u0_0, delta_0, ..., u0_{T-1}, delta_{T-1}, acc_0), G [8T, 2T + 1]:
    the speed responds to the effective accelerations a~_s = acc_0 + u0_s + dt sum_{r<s} u0_r, v_t = v_0 + dt sum_{s<t} a~_s; the
    acceleration rows bound u0_t itself (mpc_jerk.py keeps `u[0, :]` in those constraints)."""
    B, n, m = len(cfgs), 2 * T + (1 if jerk else 0), 8 * T
    G = np.zeros((m, n))
    for t in range(T - 1):
        G[2 * t, 2 * t + 3] = 1; G[2 * t, 2 * t + 1] = -1; G[2 * t + 1] = -G[2 * t]
    for t in range(T + 1):
        G[2 * T - 2 + t, 0:2 * t:2] = dt
        if jerk:
            G[2 * T - 2 + t, 2 * T] = dt * t
            for r in range(t - 1):
                G[2 * T - 2 + t, 2 * r] += dt * dt * (t - 1 - r)
        G[3 * T - 1 + t] = -G[2 * T - 2 + t]
    for t in range(T):
        G[4 * T + t, 2 * t] = 1; G[5 * T + t, 2 * t] = -1
        G[6 * T + 2 * t, 2 * t + 1] = 1; G[6 * T + 2 * t + 1, 2 * t + 1] = -1
    col = lambda f: np.array([f(e) for e in cfgs], dtype=np.float64)[:, None]
    v0, speed = np.asarray(v0, dtype=np.float64), np.asarray(speed, dtype=np.float64)
    h = np.zeros((B, m))
    h[:, :2 * T - 2] = col(lambda e: e.max_dsteer_rad * dt)
    h[:, 2 * T - 2:3 * T - 1] = (speed - v0)[:, None]
    h[:, 3 * T - 1:4 * T] = (v0 - min_speed)[:, None]
    h[:, 4 * T:5 * T] = col(lambda e: e.MAX_ACCEL)
    h[:, 5 * T:6 * T] = col(lambda e: -e.MAX_DECEL)
    h[:, 6 * T:] = max_steer
    return G, h


def kkt_check(eng, batch, dbg, cfgs=None):
    """Size-independent property: the u* the kernel returned satisfies the KKT conditions of the condensed QP the kernel built
    (strictly convex => that IS the optimum), multipliers >= 0, complementary, active bits <=> positive multipliers.
    cfgs: the per-ego configurations of a run with a table (set_ego_configs) -- the limits of ego b are then cfgs[b]'s."""
    B, T = eng.B, eng.T
    st = eng.status
    ok = st == 0
    H = dbg["H"]; H = torch.tril(H) + torch.tril(H, -1).transpose(1, 2)
    u = torch.stack([eng.oa, eng.od], dim=2).reshape(B, 2 * T)
    lam = dbg["lam"]
    n, m = 2 * T, 8 * T
    c = eng.config
    per = [c] * B if cfgs is None else cfgs
    Gn, hn = qp_constraints(T, eng.dt, batch.x0[:, 2], eng.speed.cpu().numpy(), per, c.MIN_SPEED, c.MAX_STEER_RAD)
    G, h = torch.from_numpy(Gn).to(eng.device), torch.from_numpy(hn).to(eng.device)
    stat = torch.einsum("bij,bj->bi", H, u) + dbg["g"] + lam @ G
    scale = dbg["g"].abs().amax(dim=1).clamp(min=1.0)
    assert float((stat.abs().amax(dim=1) / scale)[ok].max()) <= 1e-8
    slack = h - u @ G.T
    assert float((-slack)[ok].max()) <= 1e-8                       # primal feasible
    assert float(lam[ok].min()) >= 0.0                             # dual feasible
    assert float((lam * slack).abs()[ok].max() / float(scale.max())) <= 1e-8   # complementary
    # active bits <=> positive multipliers
    words = eng.active_mask.cpu().numpy().view(np.uint32)
    bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, -1)[:, :m].astype(bool)
    thr = (1e-9 * scale).cpu().numpy()[:, None]
    assert np.array_equal(bits[ok.cpu().numpy()], (lam.cpu().numpy() > thr)[ok.cpu().numpy()])
