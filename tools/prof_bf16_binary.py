"""tools/prof_bf16_binary.py [out.json] -- the multi-binary head on the bf16 path (PPO_ACT_MULTI_BINARY | PPO_ACT_BF16_BINARY_HEAD with compute_dtype PPO_BF16:
bf16_sample_kernel / bf16_loss_kernel<mbin>) against what such a user ran before (the generic fp32 <mbin> kernels: the same handle with PPO_F32) and beside the Gaussian
PPO_BF16 handle of the same shape (the same GEMMs, the Gaussian head forms).  256 observations, hidden [1024, 1024, 1024], 64 bits / actions.  Device time
(ppo_prof_read, all classes added) of one ppo_train_step on 4096 and on 256 rows and of one ppo_step on 8192 rows.  The three handles live in ONE process and alternate
round by round (ROUNDS rounds of REPS calls after a warm-up); a handle's figure is the median of its rounds, the spread their max - min."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

O, A, HIDDEN = 256, 64, [1024, 1024, 1024]
TRAIN_ROWS, STEP_ROWS, ROUNDS, REPS = (4096, 256), (8192,), 7, 10
HANDLES = {"generic_mbin": dict(action_dist="multi_binary"), "bf16_mbin": dict(action_dist="multi_binary", compute_dtype=1, binary_bf16_head=True),
           "bf16_gauss": dict(compute_dtype=1)}


def timed(g, call):
    g.prof_enable(True)
    for _ in range(REPS):
        call()
    p = g.prof_read()
    g.prof_enable(False)
    return sum(v[0] for v in p.values() if v[1]) / REPS * 1e3


rng = np.random.RandomState(0)
jobs = {}
for name, kw in HANDLES.items():
    g = ppo_cpp_amd.PPOHip(O, A, HIDDEN, **kw)
    g.init_orthogonal(0)
    for n in TRAIN_ROWS + STEP_ROWS:
        obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
        a, v, nlp = g.step(obs)
        b = (obs, a, rng.normal(size=n).astype(np.float32), (v + 0.3).astype(np.float32), nlp, v)
        if n in TRAIN_ROWS:
            jobs[("train", n, name)] = (g, lambda g=g, b=b: g.train_step(3e-4, 0.2, *b))
        else:
            jobs[("step", n, name)] = (g, lambda g=g, b=b: g.step(b[0]))
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
        print("%-5s %5d rows: " % (what, n) + " | ".join("%s %.1f us (spread %.1f)" % (k, med[k], spread[k]) for k in HANDLES)
              + " | bf16 / generic %.3f | mbin / gauss %.3f" % (med["bf16_mbin"] / med["generic_mbin"], med["bf16_mbin"] / med["bf16_gauss"]), flush=True)
        out["%s_rows%d" % (what, n)] = {"median_us": med, "spread_us": spread}
for (what, n, name), (g, _) in jobs.items():
    if what == "step":
        print("%s kernels: %s" % (name, {k: v for k, v in g.kernel_variants().items() if v}))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
