"""tools/prof_action_mask.py [out.json] -- what an action mask costs a categorical handle at configs[2]'s workload (4096 x 16, [256,256], 18 obs, 18 categories): device time per
kernel class (ppo_prof_read) of one ppo_train_step(_masked) on a 2048-row minibatch (B / 32), of one policy step over the 4096 environments (the launch a collect makes per
env step; ppo_collect_synthetic itself never masks) and of one ppo_update epoch of 32 minibatches (the masking handle's epoch gather also copies the masks).  A categorical
handle without masking and one with masking (random masks, every category kept with probability 1/2) alternate round by round."""
import os, sys, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

E, T, M, NMB, A, ROUNDS, REPS = 4096, 16, 2048, 32, 18, 4, 20


def make(masking):
    g = ppo_cpp_amd.PPOHip(18, A, [256, 256], action_dist="categorical")
    g.init_orthogonal(0); g.norm_init(E)
    if masking:
        g.set_action_masking(True)
    g.rollout_alloc(E, T)
    return g


def random_masks(rng, n):
    m = (rng.uniform(size=(n, A)) < 0.5).astype(np.float32)
    m[np.arange(n), rng.randint(0, A, n)] = 1.0
    return m


rng = np.random.RandomState(0)
handles = {"unmasked": make(False), "masked": make(True)}
obs_e = rng.uniform(-1, 1, (E, 18)).astype(np.float32)
mask_e = random_masks(rng, E)
obs = rng.uniform(-1, 1, (M, 18)).astype(np.float32)
mask_m = random_masks(rng, M)
batches, kw = {}, {"unmasked": {}, "masked": {"mask": mask_m}}
for name, g in handles.items():
    a, v, nlp = g.step(obs, **kw[name])
    batches[name] = (obs, a, rng.normal(size=M).astype(np.float32), (v + 0.3).astype(np.float32), nlp, v)
    g.collect_synthetic(1, 0.99, 0.95)
masks_ro = random_masks(rng, T * E).reshape(T, E, A)
acts = handles["masked"].rollout_get("actions").astype(np.int64)
masks_ro[np.arange(T)[:, None], np.arange(E)[None, :], acts] = 1.0       # the collected actions stay allowed
handles["masked"].rollout_set("masks", masks_ro)
res = {name: {"train": [], "step": [], "epoch": [], "train_kernels": {}, "epoch_kernels": {}, "counts": None} for name in handles}


def timed(g, fn):
    g.prof_enable(True)
    for _ in range(REPS):
        fn()
    p = g.prof_read()
    g.prof_enable(False)
    return {k: v[0] / REPS * 1e3 for k, v in p.items() if v[1]}


for name, g in handles.items():       # warm-up
    for _ in range(3):
        g.train_step(3e-4, 0.2, *batches[name], **kw[name])
for r in range(ROUNDS):
    for name, g in handles.items():
        train = timed(g, lambda: g.train_step(3e-4, 0.2, *batches[name], **kw[name]))
        step = timed(g, (lambda: g.step(obs_e, mask=mask_e)) if name == "masked" else (lambda: g.step(obs_e)))
        epoch = timed(g, lambda: g.update(1e-5, 0.2, 1, NMB, None, seed=r, want_rows=False))
        res[name]["train"].append(sum(train.values())); res[name]["train_kernels"] = train
        res[name]["step"].append(sum(step.values()))
        res[name]["epoch"].append(sum(epoch.values())); res[name]["epoch_kernels"] = epoch
for name, g in handles.items():
    res[name]["counts"] = {k: int(v) for k, v in g.kernel_counts().items() if v}
    print("%-9s train step %7.1f us (rounds %s)  policy step x%d %6.1f us (rounds %s)  update epoch %8.1f us (rounds %s)" % (
        name, np.median(res[name]["train"]), np.round(res[name]["train"], 1), E, np.median(res[name]["step"]), np.round(res[name]["step"], 1),
        np.median(res[name]["epoch"]), np.round(res[name]["epoch"], 1)))
    print("   train kernels (us):", {k: round(v, 1) for k, v in res[name]["train_kernels"].items()})
    print("   epoch kernels (us):", {k: round(v, 1) for k, v in res[name]["epoch_kernels"].items()})
    print("   kernels:", res[name]["counts"])
if len(sys.argv) > 1:                  # optional: the per-round numbers as JSON
    json.dump(res, open(sys.argv[1], "w"), indent=1)
