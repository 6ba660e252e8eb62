"""tools/prof_categorical.py [out.json] -- categorical vs Gaussian head at configs[2]'s workload (4096 x 16, [256,256], 18 obs, 18 actions / categories): device time per kernel class
(ppo_prof_read) of one ppo_train_step on a 2048-row minibatch (B / 32) and of one collect_synthetic; the three handles alternate round by round.
--shape_kernels adds a categorical handle created with PPO_ACT_SHAPE_KERNELS ("categorical_narrow"); --hidden 64,64 [--envs E --steps T] picks a shape where that
flag selects the narrow kernels (tools/prof_action_mask.py has the same options and also times the policy step and an update epoch).
--pair adds categorical handles created with PPO_ACT_PAIR_KERNELS ("categorical_pair": train8_kernel<cat> + weight_grad_assemble_kernel) and the masked train step of
both the flagged and the generic categorical handle (half of the categories forbidden), all alternated with the Gaussian default in the same rounds.
--bf16: the categorical head of the bf16 path instead (PPO_ACT_BF16_HEAD) at configs[4]'s shape (256 obs, 64 actions / categories, [1024,1024,1024], 8192 x 16: 4096-row
minibatches; --hidden / --envs / --steps still apply): bf16 Gaussian, bf16 categorical, bf16 categorical under a random mask (the train step; the seeded device env's collect
samples unmasked) and the wide fp32 categorical form, in alternating rounds"""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

ARGV = sys.argv[1:]
def _opt(name, default):
    if name in ARGV:
        i = ARGV.index(name); v = ARGV[i + 1]; del ARGV[i:i + 2]; return v
    return default
BF16 = "--bf16" in ARGV
if BF16:
    ARGV.remove("--bf16")
O, A = (256, 64) if BF16 else (18, 18)
HIDDEN = [int(x) for x in _opt("--hidden", "1024,1024,1024" if BF16 else "256,256").split(",")]
E, T = int(_opt("--envs", 8192 if BF16 else 4096)), int(_opt("--steps", 16))
SHAPE_KERNELS = "--shape_kernels" in ARGV
if SHAPE_KERNELS:
    ARGV.remove("--shape_kernels")
M, ROUNDS, REPS = E * T // 32, 4, 20
PAIR = "--pair" in ARGV
if PAIR:
    ARGV.remove("--pair")
MASKED = set()
VARIANTS = ([("categorical_narrow", "categorical+", {})] if SHAPE_KERNELS else []) + [("categorical", "categorical", {}), ("gaussian_generic", "gaussian", {"PPO_HIP_NO_T8": "1", "PPO_HIP_NO_DW2": "1"}), ("gaussian_default", "gaussian", {})]
if PAIR:      # "%" = PPO_ACT_PAIR_KERNELS
    VARIANTS = [("categorical_pair", "categorical%", {}), ("categorical_pair_masked", "categorical%", {}), ("categorical_masked", "categorical", {})] + VARIANTS
    MASKED = {"categorical_pair_masked", "categorical_masked"}
if BF16:      # (name, distribution, creation-time environment): "*" = compute_dtype PPO_BF16 (+ PPO_ACT_BF16_HEAD on a categorical handle)
    VARIANTS = [("bf16_gaussian", "gaussian*", {}), ("bf16_categorical", "categorical*", {}), ("bf16_categorical_masked", "categorical*", {}), ("f32_categorical_wide", "categorical", {})]
    MASKED = {"bf16_categorical_masked"}


def make(dist, env):
    for k in ("PPO_HIP_NO_T8", "PPO_HIP_NO_DW2"):
        os.environ.pop(k, None)
    os.environ.update(env)
    bf = dist.endswith("*")
    g = ppo_cpp_amd.PPOHip(O, A, HIDDEN, action_dist=dist.rstrip("+*%"), shape_kernels=dist.endswith("+"), bf16_head=bf and dist.startswith("categorical"), compute_dtype=int(bf),
                           pair_kernels=dist.endswith("%"))
    for k in env:
        os.environ.pop(k)
    g.init_orthogonal(0); g.norm_init(E); g.rollout_alloc(E, T)
    return g


def batch(g, rng, masked=False):
    obs = rng.uniform(-1, 1, (M, O)).astype(np.float32)
    if g.action_dist == "categorical":
        a = rng.randint(0, A, M).astype(np.float32)
    else:
        a = rng.normal(size=(M, A)).astype(np.float32)
    nlp, v = g.step(obs)[2], g.value(obs)
    adv = rng.normal(size=M).astype(np.float32)
    out = (obs, a, adv, (v + 0.3).astype(np.float32), nlp, v)
    if masked:                        # half of the categories forbidden, the row's own action allowed
        mask = (rng.uniform(size=(M, A)) < 0.5).astype(np.float32)
        mask[np.arange(M), a.astype(np.int64)] = 1.0
        out += (mask,)
    return out


res = {name: {"train": [], "collect": [], "train_kernels": {}, "counts": None} for name, _, _ in VARIANTS}
handles = {name: make(d, env) for name, d, env in VARIANTS}
rng = np.random.RandomState(0)
batches = {name: batch(handles[name], rng, name in MASKED) for name, _, _ in VARIANTS}
for name, g in handles.items():       # warm-up
    for _ in range(3):
        g.train_step(3e-4, 0.2, *batches[name]); g.collect_synthetic(1, 0.99, 0.95)
for r in range(ROUNDS):
    for name, g in handles.items():
        g.prof_enable(True)
        for _ in range(REPS):
            g.train_step(3e-4, 0.2, *batches[name])
        p = g.prof_read()
        g.prof_enable(True)
        for _ in range(REPS):
            g.collect_synthetic(1, 0.99, 0.95, first=False)
        q = g.prof_read()
        g.prof_enable(False)
        train = {k: v[0] / REPS * 1e3 for k, v in p.items() if v[1]}
        res[name]["train"].append(sum(train.values()))
        res[name]["train_kernels"] = train
        res[name]["collect"].append(sum(v[0] for k, v in q.items() if v[1]) / REPS * 1e3)
for name, g in handles.items():
    res[name]["counts"] = {k: int(v) for k, v in g.kernel_counts().items() if v}
    print("%-18s train step %7.1f us (rounds %s)  collect %8.1f us (rounds %s)" % (
        name, np.median(res[name]["train"]), np.round(res[name]["train"], 1), np.median(res[name]["collect"]), np.round(res[name]["collect"], 1)))
    print("   train kernels (us):", {k: round(v, 1) for k, v in res[name]["train_kernels"].items()})
    print("   kernels:", res[name]["counts"])
if ARGV:                               # optional: the per-round numbers as JSON
    json.dump(res, open(ARGV[0], "w"), indent=1)
