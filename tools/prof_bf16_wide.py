"""tools/prof_bf16_wide.py [--head categorical|binary] [out.json] -- the wide categorical head of the bf16 path (PPO_ACT_CATEGORICAL | PPO_ACT_BF16_HEAD | PPO_ACT_BF16_WIDE_HEAD with compute_dtype
PPO_BF16: bf16_logits_kernel, bf16_value_head_kernel, bf16_{sample,loss}_wide_kernel) at A = 1024 and A = 256 beside the nearest form there was before it, the
PPO_ACT_BF16_HEAD handle at A = 128 (no fp32 family holds this net).  256 observations, hidden [1024, 1024, 1024].  Device time (ppo_prof_read, all classes added,
and each class by itself) of one ppo_train_step on 4096 and on 256 rows and of one ppo_step on 8192 rows.  The three handles live in ONE process and alternate round
by round (ROUNDS rounds of REPS calls after a warm-up); a handle's figure is the median of its rounds, the spread their max - min.  The per-class figures show where
the padded value head's cost lands: train_fwd_bwd (link 0 over Ap columns), weight_grad (the vf/w tiles), grad_reduce (Adam over the padded words).
--head binary: the wide multi-binary head (PPO_ACT_MULTI_BINARY | PPO_ACT_BF16_BINARY_HEAD | PPO_ACT_BF16_WIDE_BINARY_HEAD: bf16_{sample,loss}_wide_binary_kernel) at
A = 1024 and A = 256, in the SAME process and rounds the wide categorical handle at the same A and the 128-bit PPO_ACT_BF16_BINARY_HEAD handle.
Per-kernel times (the logits product against a hidden layer's share of gemm_chain_bf16_kernel, the three row kernels) come from a kernel trace of this script."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

O, HIDDEN = 256, [1024, 1024, 1024]
TRAIN_ROWS, STEP_ROWS, ROUNDS, REPS = (4096, 256), (8192,), 7, 10
CAT, BIN = dict(action_dist="categorical", bf16_head=True), dict(action_dist="multi_binary", binary_bf16_head=True)
HANDLES = {"cat_A128": (128, CAT), "wide_A256": (256, dict(CAT, bf16_wide_head=True)), "wide_A1024": (1024, dict(CAT, bf16_wide_head=True))}
args = sys.argv[1:]
if "--head" in args:
    head = args.pop(args.index("--head") + 1)
    args.remove("--head")
    if head == "binary":
        HANDLES = {"mbin_A128": (128, BIN), "wide_A256": HANDLES["wide_A256"], "wbin_A256": (256, dict(BIN, binary_bf16_wide_head=True)),
                   "wide_A1024": HANDLES["wide_A1024"], "wbin_A1024": (1024, dict(BIN, binary_bf16_wide_head=True))}
    elif head != "categorical":
        sys.exit("--head takes categorical or binary, not %r" % head)


def timed(g, call):
    g.prof_enable(True)
    for _ in range(REPS):
        call()
    p = g.prof_read()
    g.prof_enable(False)
    return {k: v[0] / REPS * 1e3 for k, v in p.items() if v[1]}


rng = np.random.RandomState(0)
jobs = {}
for name, (A, kw) in HANDLES.items():
    g = ppo_cpp_amd.PPOHip(O, A, HIDDEN, compute_dtype=1, **kw)
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
        tot = {name: [sum(r.values()) for r in res[(what, n, name)]] for name in HANDLES}
        med = {name: float(np.median(tot[name])) for name in HANDLES}
        spread = {name: float(np.ptp(tot[name])) for name in HANDLES}
        print("%-5s %5d rows: " % (what, n) + " | ".join("%s %.1f us (spread %.1f)" % (k, med[k], spread[k]) for k in HANDLES), flush=True)
        classes = sorted(set(k for name in HANDLES for r in res[(what, n, name)] for k in r))
        per = {c: {name: float(np.median([r.get(c, 0.0) for r in res[(what, n, name)]])) for name in HANDLES} for c in classes}
        for c in classes:
            print("      %-14s " % c + " | ".join("%.1f" % per[c][k] for k in HANDLES), flush=True)
        out["%s_rows%d" % (what, n)] = {"median_us": med, "spread_us": spread, "class_median_us": per}
for (what, n, name), (g, _) in jobs.items():
    if what == "step":
        print("%s kernels: %s" % (name, {k: v for k, v in g.kernel_variants().items() if v}))
if args:
    json.dump(out, open(args[0], "w"), indent=1)
