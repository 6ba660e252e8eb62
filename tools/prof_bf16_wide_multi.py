"""tools/prof_bf16_wide_multi.py [out.json] -- the wide multi-categorical head of the bf16 path (ppo_create_multi_ex with PPO_ACT_BF16_MULTI_HEAD |
PPO_ACT_BF16_WIDE_MULTI_HEAD, PPO_BF16: bf16_{sample,loss}_wide_multi_kernel) at 1024 logits cut as nvec = (64,) x 16, (256,) x 4 and (1024,), beside the wide
CATEGORICAL handle at A = 1024 (PPO_ACT_BF16_WIDE_HEAD), and -- for the cost of a component in the 128-wide walk, re-measured in the same run -- the
PPO_ACT_BF16_MULTI_HEAD handle with nvec = (8,) x 16 beside the PPO_ACT_BF16_HEAD categorical handle at A = 128.  256 observations, hidden [1024, 1024, 1024].
Device time (ppo_prof_read, all classes added) of one ppo_train_step on 4096 and on 256 rows and of one ppo_step on 8192 rows.  All handles live in ONE process and
alternate round by round (ROUNDS rounds of REPS calls after a warm-up); a handle's figure is the median of its rounds, the spread their max - min.
The quantity of interest is the cost per component: (K = 16 minus K = 1) / 15 of the batched walk against (nvec = (8,) x 16 minus A = 128) / 15 of the 128-wide one."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

O, HIDDEN = 256, [1024, 1024, 1024]
TRAIN_ROWS, STEP_ROWS, ROUNDS, REPS = (4096, 256), (8192,), 7, 10
CAT, MULTI = dict(action_dist="categorical"), dict(action_dist="multi_categorical", multi_bf16_wide_head=True)
HANDLES = {"wcat_A1024": (1024, dict(CAT, bf16_wide_head=True)), "wmcat_1x1024": (None, dict(MULTI, nvec=[1024])), "wmcat_4x256": (None, dict(MULTI, nvec=[256] * 4)),
           "wmcat_16x64": (None, dict(MULTI, nvec=[64] * 16)), "cat_A128": (128, CAT), "mcat_16x8": (None, dict(MULTI, nvec=[8] * 16))}


def timed(g, call):
    g.prof_enable(True)
    for _ in range(REPS):
        call()
    p = g.prof_read()
    g.prof_enable(False)
    return sum(v[0] for v in p.values() if v[1]) / REPS * 1e3


rng = np.random.RandomState(0)
jobs = {}
for name, (A, kw) in HANDLES.items():
    g = ppo_cpp_amd.PPOHip(O, A, HIDDEN, compute_dtype=1, bf16_head=True, **kw)
    g.init_orthogonal(0)
    for n in TRAIN_ROWS + STEP_ROWS:
        obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
        a, v, nlp = g.step(obs)
        b = (obs, a, rng.normal(size=n).astype(np.float32), (v + 0.3).astype(np.float32), nlp, v)
        jobs[("train" if n in TRAIN_ROWS else "step", n, name)] = (g, (lambda g=g, b=b: g.train_step(3e-4, 0.2, *b)) if n in TRAIN_ROWS else (lambda g=g, b=b: g.step(b[0])))
for g, call in jobs.values():
    for _ in range(5):
        call()
res = {key: [] for key in jobs}
for r in range(ROUNDS):
    for key, (g, call) in jobs.items():
        res[key].append(timed(g, call))
out = {}
for what, rows in (("train", TRAIN_ROWS), ("step", STEP_ROWS)):
    for n in rows:
        med = {name: float(np.median(res[(what, n, name)])) for name in HANDLES}
        spread = {name: float(np.ptp(res[(what, n, name)])) for name in HANDLES}
        per = {"batched walk": (med["wmcat_16x64"] - med["wmcat_1x1024"]) / 15, "128-wide walk": (med["mcat_16x8"] - med["cat_A128"]) / 15}
        print("%-5s %5d rows: " % (what, n) + " | ".join("%s %.1f us (spread %.1f)" % (k, med[k], spread[k]) for k in HANDLES), flush=True)
        print("      us per component: " + " | ".join("%s %.2f" % kv for kv in per.items()), flush=True)
        out["%s_rows%d" % (what, n)] = {"median_us": med, "spread_us": spread, "us_per_component": per}
for (what, n, name), (g, _) in jobs.items():
    if what == "step":
        print("%s kernels: %s" % (name, {k: v for k, v in g.kernel_variants().items() if v}))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
