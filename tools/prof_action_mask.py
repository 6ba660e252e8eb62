"""tools/prof_action_mask.py [out.json] -- what an action mask costs a categorical handle at configs[2]'s workload (4096 x 16, [256,256], 18 obs, 18 categories): device time per
kernel class (ppo_prof_read) of one ppo_train_step(_masked) on a 2048-row minibatch (B / 32), of one policy step over the 4096 environments (the launch a collect makes per
env step; ppo_collect_synthetic itself never masks) and of one ppo_update epoch of 32 minibatches (the masking handle's epoch gather also copies the masks).  A categorical
handle without masking and one with masking (random masks, every category kept with probability 1/2) alternate round by round.
Options: --envs E --steps T --hidden 64,64 choose another workload (configs[3]: --envs 1024 --steps 64 --hidden 64,64; configs[1]: --envs 1 --steps 2048 --hidden 64,64);
--shape_kernels adds the same two handles created with PPO_ACT_SHAPE_KERNELS ("narrow_unmasked", "narrow_masked"); --gaussian adds a Gaussian handle of the shape
with PPO_HIP_NO_LAZY_ADAM=1 (train launch + reduce + adam_kernel per step, for scale).  Beside the device time per kernel class every figure has the host's wall
time per call behind it ("wall": launches and the gaps between them included)."""
import os, sys, json, time, argparse
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--hidden", default="256,256")
ap.add_argument("--shape_kernels", action="store_true")
ap.add_argument("--gaussian", action="store_true")
ap.add_argument("--rounds", type=int, default=4)
args = ap.parse_args()
E, T, NMB, A, ROUNDS, REPS = args.envs, args.steps, 32, 18, args.rounds, 20
M = E * T // NMB
HIDDEN = [int(x) for x in args.hidden.split(",")]


def make(masking, shape_kernels=False, dist="categorical"):
    if dist == "gaussian":
        os.environ["PPO_HIP_NO_LAZY_ADAM"] = "1"
    g = ppo_cpp_amd.PPOHip(18, A, HIDDEN, action_dist=dist, shape_kernels=shape_kernels)
    os.environ.pop("PPO_HIP_NO_LAZY_ADAM", None)
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
if args.shape_kernels:
    handles.update({"narrow_unmasked": make(False, True), "narrow_masked": make(True, True)})
if args.gaussian:
    handles["gaussian"] = make(False, dist="gaussian")
MASKED = [n for n in handles if n.endswith("masked") and not n.endswith("unmasked")]
obs_e = rng.uniform(-1, 1, (E, 18)).astype(np.float32)
mask_e = random_masks(rng, E)
obs = rng.uniform(-1, 1, (M, 18)).astype(np.float32)
mask_m = random_masks(rng, M)
batches, kw = {}, {n: ({"mask": mask_m} if n in MASKED else {}) for n in handles}
for name, g in handles.items():
    a, v, nlp = g.step(obs, **kw[name])
    batches[name] = (obs, a, rng.normal(size=M).astype(np.float32), (v + 0.3).astype(np.float32), nlp, v)
    g.collect_synthetic(1, 0.99, 0.95)
masks_ro = random_masks(rng, T * E).reshape(T, E, A)
for name in MASKED:
    acts = handles[name].rollout_get("actions").astype(np.int64)
    mr = masks_ro.copy()
    mr[np.arange(T)[:, None], np.arange(E)[None, :], acts] = 1.0       # the collected actions stay allowed
    handles[name].rollout_set("masks", mr)
res = {name: {"train": [], "step": [], "epoch": [], "train_wall": [], "step_wall": [], "epoch_wall": [], "train_kernels": {}, "epoch_kernels": {}, "counts": None} for name in handles}


def timed(g, fn):
    """(device time per kernel class, host wall time per call without the profiler's events), us"""
    g.prof_enable(True)
    for _ in range(REPS):
        fn()
    p = g.prof_read()
    g.prof_enable(False)
    g.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    g.sync()
    wall = (time.perf_counter() - t0) / REPS * 1e6
    return {k: v[0] / REPS * 1e3 for k, v in p.items() if v[1]}, wall


for name, g in handles.items():       # warm-up
    for _ in range(3):
        g.train_step(3e-4, 0.2, *batches[name], **kw[name])
for r in range(ROUNDS):
    for name, g in handles.items():
        train, tw = timed(g, lambda: g.train_step(3e-4, 0.2, *batches[name], **kw[name]))
        step, sw = timed(g, (lambda: g.step(obs_e, mask=mask_e)) if name in MASKED else (lambda: g.step(obs_e)))
        epoch, ew = timed(g, lambda: g.update(1e-5, 0.2, 1, NMB, None, seed=r, want_rows=False))
        res[name]["train_wall"].append(tw); res[name]["step_wall"].append(sw); res[name]["epoch_wall"].append(ew)
        res[name]["train"].append(sum(train.values())); res[name]["train_kernels"] = train
        res[name]["step"].append(sum(step.values()))
        res[name]["epoch"].append(sum(epoch.values())); res[name]["epoch_kernels"] = epoch
for name, g in handles.items():
    res[name]["counts"] = {k: int(v) for k, v in g.kernel_counts().items() if v}
    print("%-15s train step %7.1f us (rounds %s)  policy step x%d %6.1f us (rounds %s)  update epoch %8.1f us (rounds %s)" % (
        name, np.median(res[name]["train"]), np.round(res[name]["train"], 1), E, np.median(res[name]["step"]), np.round(res[name]["step"], 1),
        np.median(res[name]["epoch"]), np.round(res[name]["epoch"], 1)))
    print("   wall per call (us): train step %.1f  policy step %.1f  update epoch %.1f" % (
        np.median(res[name]["train_wall"]), np.median(res[name]["step_wall"]), np.median(res[name]["epoch_wall"])))
    print("   train kernels (us):", {k: round(v, 1) for k, v in res[name]["train_kernels"].items()})
    print("   epoch kernels (us):", {k: round(v, 1) for k, v in res[name]["epoch_kernels"].items()})
    print("   kernels:", res[name]["counts"])
if args.out:                           # optional: the per-round numbers as JSON
    json.dump(res, open(args.out, "w"), indent=1)
