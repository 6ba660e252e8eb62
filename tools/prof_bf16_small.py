"""tools/prof_bf16_small.py [out.json] -- the small-batch forward of the bf16 path (ppo_set_bf16_small_step: bf16_small_forward_kernel<RT> in the place of one 128-row tile
GEMM launch per hidden layer) at the benchmark's wide net: 256 observations, hidden [1024, 1024, 1024].
  (a) device time (ppo_prof_read, class policy_step) of one ppo_step on the Gaussian PPO_BF16 handle (64 actions) at 1, 16, 32 and 64 rows, setting off against on: TWO
      handles in ONE process, alternating round by round (ROUNDS rounds of REPS calls after a warm-up); a figure is the median of its rounds, the spread their max - min;
  (b) the same on the wide categorical handle (A = 1024) at 64 rows;
  (c) wall time per env step of a ppo_rollout_act / ppo_rollout_observe loop behind a stand-in host Env (a seeded array per step, no simulation) at 1 and 64
      environments, T = 64 steps per rollout, same alternation.
The outputs of the two handles are compared bit for bit on the way (the setting changes no bit)."""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

O, HIDDEN, ROWS, ROUNDS, REPS, T = 256, [1024, 1024, 1024], (1, 16, 32, 64), 7, 20, 64
WCAT = dict(action_dist="categorical", bf16_head=True, bf16_wide_head=True)
rng = np.random.RandomState(0)


def pair(A, **kw):
    gs = {}
    for name in ("off", "on"):
        g = ppo_cpp_amd.PPOHip(O, A, HIDDEN, compute_dtype=1, **kw)
        g.init_orthogonal(0)
        g.set_bf16_small_step(name == "on")
        gs[name] = g
    return gs


def timed(g, call):
    g.prof_enable(True)
    for _ in range(REPS):
        call()
    p = g.prof_read()
    g.prof_enable(False)
    return sum(v[0] for v in p.values() if v[1]) / REPS * 1e3


def rollout(g, E, raw, rew, dn):
    t0 = time.perf_counter()
    for t in range(T):
        g.rollout_act(t)
        g.rollout_observe(t, raw[t + 1], rew[t], dn[t])
    return (time.perf_counter() - t0) / T * 1e6


def report(tag, res, out):
    med, spread = {k: float(np.median(v)) for k, v in res.items()}, {k: float(np.ptp(v)) for k, v in res.items()}
    print("%-28s off %.1f us (spread %.1f) | on %.1f us (spread %.1f) | off / on %.2f" % (tag, med["off"], spread["off"], med["on"], spread["on"], med["off"] / med["on"]), flush=True)
    out[tag] = {"median_us": med, "spread_us": spread}


out = {}
for label, A, kw, rows in (("gauss_A64", 64, {}, ROWS), ("wcat_A1024", 1024, WCAT, (64,))):
    gs = pair(A, **kw)
    for n in rows:
        obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
        noise = (rng.normal(size=(n, A)) if not kw else np.clip(rng.uniform(size=(n, A)), 1e-6, 1 - 1e-6)).astype(np.float32)
        for x, y in zip(gs["off"].step(obs, noise), gs["on"].step(obs, noise)):
            assert np.array_equal(x, y), "the setting changed a bit"
        for g in gs.values():
            for _ in range(5):
                g.step(obs)
        res = {"off": [], "on": []}
        for r in range(ROUNDS):
            for name, g in gs.items():
                res[name].append(timed(g, lambda: g.step(obs)))
        report("%s step %2d rows" % (label, n), res, out)
    print("%s kernels (on): %s" % (label, {k: v for k, v in gs["on"].kernel_variants().items() if v}), flush=True)
for E in (1, 64):
    gs = pair(64)
    raw, rew, dn = rng.uniform(-1, 1, (T + 1, E, O)).astype(np.float32), rng.uniform(-1, 1, (T, E)).astype(np.float32), np.zeros((T, E), np.float32)
    res = {"off": [], "on": []}
    for g in gs.values():
        g.norm_init(E); g.rollout_alloc(E, T); g.rollout_reset(raw[0])
        rollout(g, E, raw, rew, dn); g.rollout_finish(0.99, 0.95)
    for r in range(ROUNDS):
        for name, g in gs.items():
            g.rollout_reset(raw[0])
            res[name].append(rollout(g, E, raw, rew, dn))
            g.rollout_finish(0.99, 0.95)
    report("host Env loop, %2d envs (wall)" % E, res, out)
if sys.argv[1:]:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
