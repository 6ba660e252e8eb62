"""tools/prof_pair_multi.py [out.json] -- the multi-categorical head in the [256,256] kernel pair (ppo_create_multi_ex with PPO_ACT_PAIR_KERNELS: train8_kernel<mcat> +
weight_grad_assemble_kernel) against the generic <mcat> kernels (the same handle without the flag) and beside the flagged categorical handle (train8_kernel<cat>) with
act_dim = sum(nvec): device time per kernel class (ppo_prof_read) of one ppo_train_step on 64 and on 2048 rows at (18 observations, nvec = (6, 6, 6)), and, for the
component walk's cost at its longest, at (50 observations, nvec = (4,) x 16).  All handles live in ONE process and alternate round by round (ROUNDS rounds of REPS
calls after a warm-up); the figure of a handle is the median of its rounds, the spread their max - min."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

HIDDEN = [256, 256]
SHAPES = [(18, (6, 6, 6)), (50, (4,) * 16)]
TRAIN_ROWS, ROUNDS, REPS = (64, 2048), 5, 40
NAMES = ("generic_mcat", "pair_mcat", "pair_mcat_masked", "pair_cat")


def make(name, O, nvec):
    if name == "pair_cat":
        g = ppo_cpp_amd.PPOHip(O, sum(nvec), HIDDEN, action_dist="categorical", pair_kernels=True)
    else:
        g = ppo_cpp_amd.PPOHip(O, None, HIDDEN, action_dist="multi_categorical", nvec=list(nvec), pair_kernels=name != "generic_mcat")
    g.init_orthogonal(0)
    return g


def batch(g, rng, n, O, nvec, masked):
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    if g.action_dist == "categorical":
        a = rng.randint(0, sum(nvec), n).astype(np.float32)
    else:
        a = np.stack([rng.randint(0, nk, n) for nk in nvec], 1).astype(np.float32)
    nlp, v = g.step(obs)[2], g.value(obs)
    out = (obs, a, rng.normal(size=n).astype(np.float32), (v + 0.3).astype(np.float32), nlp, v)
    if masked:                         # half of the categories forbidden, every component's own action allowed
        mask = (rng.uniform(size=(n, sum(nvec))) < 0.5).astype(np.float32)
        off = np.concatenate([[0], np.cumsum(nvec)[:-1]])
        mask[np.arange(n)[:, None], (a.astype(np.int64) + off)] = 1.0
        out += (mask,)
    return out


def timed(g, call):
    """device microseconds per call, by kernel class"""
    g.prof_enable(True)
    for _ in range(REPS):
        call()
    p = g.prof_read()
    g.prof_enable(False)
    return {k: v[0] / REPS * 1e3 for k, v in p.items() if v[1]}


rng = np.random.RandomState(0)
jobs, handles = {}, {}
for O, nvec in SHAPES:
    for name in NAMES:
        g = handles[(O, nvec, name)] = make(name, O, nvec)
        for n in TRAIN_ROWS:
            b = batch(g, rng, n, O, nvec, name.endswith("masked"))
            jobs[(O, nvec, n, name)] = (g, lambda g=g, b=b: g.train_step(3e-4, 0.2, *b[:6], **({"mask": b[6]} if len(b) > 6 else {})))
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
for O, nvec in SHAPES:
    for n in TRAIN_ROWS:
        med = {name: float(np.median(res[(O, nvec, n, name)]["rounds"])) for name in NAMES}
        spread = {name: float(np.ptp(res[(O, nvec, n, name)]["rounds"])) for name in NAMES}
        print("O %d nvec %s, %5d rows: " % (O, list(nvec), n) + " | ".join("%s %.2f us (spread %.2f)" % (name, med[name], spread[name]) for name in NAMES)
              + " | pair / generic %.3f" % (med["pair_mcat"] / med["generic_mcat"]))
        for name in NAMES:
            print("      %-16s classes (us): %s" % (name, res[(O, nvec, n, name)]["classes"]))
        out["O%d_K%d_rows%d" % (O, len(nvec), n)] = {"median_us": med, "spread_us": spread, "classes_us": {name: res[(O, nvec, n, name)]["classes"] for name in NAMES}}
for key, g in handles.items():
    print("%s kernels: %s" % (key, {k: int(v) for k, v in g.kernel_counts().items() if v}))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
