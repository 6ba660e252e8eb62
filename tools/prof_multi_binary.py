"""tools/prof_multi_binary.py [out.json] -- the multi-binary head beside the categorical ones on the generic fp32 kernels: device time (ppo_prof_read) of the policy
step at 16 / 1024 rows and of the train step at 64 / 2048 rows, at (18 obs, 18 logits, [256,256]) and (18, 18, [64,64]).
Handles, all without flags (policy_step_kernel / train_fwd_bwd_kernel<mbin | cat | mcat>): "multi_binary" (18 bits), "categorical" (18 categories) and
"multi_categorical" with nvec = (2,) * 16 (32 logits: 16 on / off decisions the way a multi-categorical handle states them); and "multi_binary_narrow", the
multi-binary handle created with binary_shape_kernels=True (PPO_ACT_BINARY_SHAPE_KERNELS): narrow_step_kernel / narrow_train_kernel<mbin> at [64,64], the generic
<mbin> kernels again at [256,256], where the flag does not take effect; and "multi_binary_pair", the multi-binary handle created with binary_pair_kernels=True
(PPO_ACT_BINARY_PAIR_KERNELS): train8_kernel<mbin> + weight_grad_assemble_kernel at [256,256], the generic <mbin> kernels again at [64,64] (the "kernels" line,
read from kernel_variants(), says which ran; both flagged handles keep policy_step_kernel<mbin> wherever their flag does not move the act side).  One process; the handles alternate round by
round; every (handle, rows) pair is warmed up before the timed rounds.  Per call: the policy_step class, the train_fwd_bwd class and the whole train step (all
classes), in microseconds, median over the rounds with the rounds' values beside it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

O, ROUNDS, REPS = 18, 5, 50
SHAPES = ([256, 256], [64, 64])
STEP_ROWS, TRAIN_ROWS = (16, 1024), (64, 2048)
HANDLES = (("multi_binary", dict(act_dim=18, action_dist="multi_binary")), ("multi_binary_narrow", dict(act_dim=18, action_dist="multi_binary", binary_shape_kernels=True)),
           ("multi_binary_pair", dict(act_dim=18, action_dist="multi_binary", binary_pair_kernels=True)),
           ("categorical", dict(act_dim=18, action_dist="categorical")),
           ("multi_categorical", dict(act_dim=None, action_dist="multi_categorical", nvec=(2,) * 16)))


def make(hidden, kw):
    kw = dict(kw)
    g = ppo_cpp_amd.PPOHip(O, kw.pop("act_dim"), hidden, **kw)
    g.init_orthogonal(0)
    return g


def batch(g, rng, n):
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    a, v, nlp = g.step(obs)                       # the handle's own actions: valid for every head
    adv = rng.normal(size=n).astype(np.float32)
    return obs, a, adv, (v + 0.3).astype(np.float32), nlp, v


def timed(g, call):
    g.prof_enable(True)
    for _ in range(REPS):
        call()
    p = g.prof_read()
    g.prof_enable(False)
    return {k: v[0] / REPS * 1e3 for k, v in p.items() if v[1]}


def main():
    rng = np.random.RandomState(0)
    out = {}
    for hidden in SHAPES:
        handles = {name: make(hidden, kw) for name, kw in HANDLES}
        obs = {n: rng.uniform(-1, 1, (n, O)).astype(np.float32) for n in STEP_ROWS}
        batches = {(name, n): batch(g, rng, n) for name, g in handles.items() for n in TRAIN_ROWS}
        res = {name: {"step": {n: [] for n in STEP_ROWS}, "train_fb": {n: [] for n in TRAIN_ROWS}, "train": {n: [] for n in TRAIN_ROWS}} for name in handles}
        for name, g in handles.items():           # warm-up of every shape the timed rounds use
            for _ in range(3):
                for n in STEP_ROWS:
                    g.step(obs[n])
                for n in TRAIN_ROWS:
                    g.train_step(3e-4, 0.2, *batches[name, n])
        for _ in range(ROUNDS):
            for name, g in handles.items():
                for n in STEP_ROWS:
                    res[name]["step"][n].append(timed(g, lambda: g.step(obs[n]))["policy_step"])
                for n in TRAIN_ROWS:
                    t = timed(g, lambda: g.train_step(3e-4, 0.2, *batches[name, n]))
                    res[name]["train_fb"][n].append(t["train_fwd_bwd"])
                    res[name]["train"][n].append(sum(t.values()))
        print("hidden %s" % hidden)
        for name, g in handles.items():
            r = res[name]
            print("  %-20s policy step %s | train_fwd_bwd %s | train step %s   (us, median of %d rounds x %d calls)" % (
                name, " ".join("%d rows %.2f" % (n, np.median(r["step"][n])) for n in STEP_ROWS), " ".join("%d rows %.2f" % (n, np.median(r["train_fb"][n])) for n in TRAIN_ROWS),
                " ".join("%d rows %.2f" % (n, np.median(r["train"][n])) for n in TRAIN_ROWS), ROUNDS, REPS))
            print("     rounds: step %s train_fwd_bwd %s train step %s" % tuple({n: np.round(v, 2).tolist() for n, v in r[k].items()} for k in ("step", "train_fb", "train")))
            print("     kernels:", {k: int(v) for k, v in g.kernel_variants().items() if v})
            g.close()
        out[",".join(map(str, hidden))] = {name: {k: {str(n): v for n, v in d.items()} for k, d in r.items()} for name, r in res.items()}
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
