"""tools/prof_narrow_multi.py [out.json] -- the multi-categorical head on the narrow kernels (ppo_create_multi_ex with PPO_ACT_SHAPE_KERNELS) against the generic <mcat>
kernels (the same handle without the flag) at (18 observations, nvec = (6, 6, 6), [64, 64]): device time per kernel class (ppo_prof_read) of one ppo_train_step on
64 and on 2048 rows and of one policy step on 16 and on 1024 rows.  Both handles live in ONE process and alternate round by round (ROUNDS rounds of REPS calls
after a warm-up); the figure of a handle is the median of its rounds, the spread their max - min.  The unflagged train step is train_fwd_bwd + weight_grad +
grad_reduce + adam, the flagged one train_fwd_bwd + grad_reduce + adam (narrow_train_kernel + narrow_reduce_kernel + adam_kernel)."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

O, NVEC, HIDDEN = 18, (6, 6, 6), [64, 64]
TRAIN_ROWS, STEP_ROWS, ROUNDS, REPS = (64, 2048), (16, 1024), 5, 60
K, A = len(NVEC), sum(NVEC)


def batch(g, rng, n):
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    a = np.stack([rng.randint(0, nk, n) for nk in NVEC], 1).astype(np.float32)
    nlp, v = g.step(obs)[2], g.value(obs)
    return obs, a, rng.normal(size=n).astype(np.float32), (v + 0.3).astype(np.float32), nlp, v


def timed(g, call):
    """device microseconds per call, by kernel class"""
    g.prof_enable(True)
    for _ in range(REPS):
        call()
    p = g.prof_read()
    g.prof_enable(False)
    return {k: v[0] / REPS * 1e3 for k, v in p.items() if v[1]}


handles = {"generic": ppo_cpp_amd.PPOHip(O, None, HIDDEN, action_dist="multi_categorical", nvec=list(NVEC)),
           "narrow": ppo_cpp_amd.PPOHip(O, None, HIDDEN, action_dist="multi_categorical", nvec=list(NVEC), shape_kernels=True)}
rng = np.random.RandomState(0)
for g in handles.values():
    g.init_orthogonal(0)
jobs = {}
for n in TRAIN_ROWS:
    for name, g in handles.items():
        b = batch(g, rng, n)
        jobs[("train", n, name)] = (g, lambda g=g, b=b: g.train_step(3e-4, 0.2, *b))
for n in STEP_ROWS:
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    for name, g in handles.items():
        jobs[("step", n, name)] = (g, lambda g=g, obs=obs: g.step(obs))
for g, call in jobs.values():          # warm-up
    for _ in range(10):
        call()
res = {key: {"rounds": [], "classes": None} for key in jobs}
for r in range(ROUNDS):
    for key, (g, call) in jobs.items():
        t = timed(g, call)
        res[key]["rounds"].append(sum(t.values()))
        res[key]["classes"] = {k: round(v, 2) for k, v in t.items()}
out = {}
for what, rows in (("train", TRAIN_ROWS), ("step", STEP_ROWS)):
    for n in rows:
        med = {name: float(np.median(res[(what, n, name)]["rounds"])) for name in handles}
        spread = {name: float(np.ptp(res[(what, n, name)]["rounds"])) for name in handles}
        print("%-5s %5d rows: generic %7.2f us (spread %.2f) | narrow %7.2f us (spread %.2f) | narrow / generic %.3f" % (
            what, n, med["generic"], spread["generic"], med["narrow"], spread["narrow"], med["narrow"] / med["generic"]))
        for name in handles:
            print("      %-8s classes (us): %s" % (name, res[(what, n, name)]["classes"]))
        out["%s_%d" % (what, n)] = {"median_us": med, "spread_us": spread, "classes_us": {name: res[(what, n, name)]["classes"] for name in handles}}
for name, g in handles.items():
    print("%-8s kernels: %s" % (name, {k: int(v) for k, v in g.kernel_counts().items() if v}))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
