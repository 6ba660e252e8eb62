"""tools/prof_bf16_multi.py [out.json] -- the multi-categorical head on the bf16 path (ppo_create_multi_ex with PPO_ACT_BF16_MULTI_HEAD and compute_dtype PPO_BF16:
bf16_sample_kernel / bf16_loss_kernel<mcat[,mask]>) against what such a user ran before (the generic fp32 <mcat> kernels: the same handle with PPO_F32) and beside the
floor (the categorical PPO_BF16 handle with act_dim = sum(nvec): the same GEMMs, one walk instead of K).  BASELINE configs[4]'s net (256 observations, hidden
[1024, 1024, 1024]) with nvec = (16, 16, 16, 16) -- A = 64, that config's action width -- and, for the component walk at its longest, nvec = (8,) x 16 -- A = 128.
Device time per kernel class (ppo_prof_read) of one ppo_train_step on 4096 rows (that config's minibatch) and on 256, and of one ppo_step on 8192 and on 64 rows.
All handles live in ONE process and alternate round by round (ROUNDS rounds of REPS calls after a warm-up); the figure of a handle is the median of its rounds, the
spread their max - min.  The generic fp32 family cannot hold this net with 128 logits (ppo_create_multi refuses it: the two-tile LDS layout needs 170512 bytes), so
its column is "n/a" at nvec = (8,) x 16: the message is printed.  The loss kernel has no class of its own: it runs inside
"train_fwd_bwd" (forward GEMMs, heads, loss, backward links).  The per-class figures printed (and written to out.json) are the LAST round's, not medians."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

O, HIDDEN = 256, [1024, 1024, 1024]
SHAPES = [(HIDDEN, nvec) for nvec in [(16,) * 4, (8,) * 16]]
TRAIN_ROWS, STEP_ROWS, ROUNDS, REPS = (4096, 256), (8192, 64), 5, 10
NAMES = ("generic_mcat", "bf16_mcat", "bf16_mcat_masked", "bf16_cat")


def make(name, hid, nvec):
    """the handle, or None where the family cannot hold the net (the message is printed)"""
    try:
        if name == "bf16_cat":
            g = ppo_cpp_amd.PPOHip(O, sum(nvec), hid, action_dist="categorical", compute_dtype=1, bf16_head=True)
        else:
            bf = name != "generic_mcat"
            g = ppo_cpp_amd.PPOHip(O, None, hid, action_dist="multi_categorical", nvec=list(nvec), compute_dtype=int(bf), bf16_head=bf)
    except ppo_cpp_amd.PPOHipError as e:
        print("%s at hidden %s, nvec %s: not created: %s" % (name, hid, list(nvec), e))
        return None
    g.init_orthogonal(0)
    return g


def batch(g, rng, n, nvec, masked):
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
for hid, nvec in SHAPES:
    for name in NAMES:
        g = handles[(len(hid), nvec, name)] = make(name, hid, nvec)
        if g is None:
            continue
        masked = name.endswith("masked")
        for n in TRAIN_ROWS:
            b = batch(g, rng, n, nvec, masked)
            jobs[("train", len(hid), nvec, n, name)] = (g, lambda g=g, b=b: g.train_step(3e-4, 0.2, *b[:6], **({"mask": b[6]} if len(b) > 6 else {})))
        for n in STEP_ROWS:
            b = batch(g, rng, n, nvec, masked)
            jobs[("step", len(hid), nvec, n, name)] = (g, lambda g=g, b=b: g.step(b[0], **({"mask": b[6]} if len(b) > 6 else {})))
for g, call in jobs.values():          # warm-up
    for _ in range(5):
        call()
res = {key: {"rounds": [], "classes": None} for key in jobs}
for r in range(ROUNDS):
    for key, (g, call) in jobs.items():
        t = timed(g, call)
        res[key]["rounds"].append(sum(t.values()))
        res[key]["classes"] = {k: round(v, 2) for k, v in t.items()}
out = {}
for hid, nvec in SHAPES:
    for what, rows in (("train", TRAIN_ROWS), ("step", STEP_ROWS)):
        for n in rows:
            have = [name for name in NAMES if (what, len(hid), nvec, n, name) in res]
            med = {name: float(np.median(res[(what, len(hid), nvec, n, name)]["rounds"])) for name in have}
            spread = {name: float(np.ptp(res[(what, len(hid), nvec, n, name)]["rounds"])) for name in have}
            ratio = "%.3f" % (med["bf16_mcat"] / med["generic_mcat"]) if "generic_mcat" in med else "n/a"
            print("%-5s L %d K %2d A %3d, %5d rows: " % (what, len(hid), len(nvec), sum(nvec), n)
                  + " | ".join("%s %.2f us (spread %.2f)" % (name, med[name], spread[name]) if name in med else "%s n/a" % name for name in NAMES)
                  + " | bf16 / generic %s | mcat / cat %.3f" % (ratio, med["bf16_mcat"] / med["bf16_cat"]))
            for name in have:
                print("      %-16s classes (us): %s" % (name, res[(what, len(hid), nvec, n, name)]["classes"]))
            out["%s_L%d_K%d_rows%d" % (what, len(hid), len(nvec), n)] = {"median_us": med, "spread_us": spread,
                                                                         "classes_us": {name: res[(what, len(hid), nvec, n, name)]["classes"] for name in have}}
for key, g in handles.items():
    if g is not None:
        print("%s kernels: %s" % (key, {k: int(v) for k, v in g.kernel_counts().items() if v}))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
