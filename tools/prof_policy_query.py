"""tools/prof_policy_query.py [out.json] -- what a policy query costs beside the policy step on the same handle and rows: device time per launch (ppo_prof_read,
class policy_step) of evaluate_actions (policy_eval_kernel) against step (policy_step_kernel, or narrow_step_kernel where the handle's step runs the narrow family)
at 1024 and 4096 rows, and of rollout_evaluate at configs[2]'s 4096 environments x 16 steps against a step over the same 65536 rows in one call (the same
yardstick at the batch's size); the whole collect_synthetic of that rollout, ALL kernel classes added up (its policy steps are booked under other classes where a
one-launch rollout form serves the handle), stands beside them for scale.
Shapes (18 obs, 18 actions, [256,256]) and (18, 6, [64,64]); Gaussian and categorical handles, all without flags.  One process; step and query alternate round by round
on every handle; every (handle, rows) pair is warmed up before the timed rounds.  Microseconds, median over the rounds with the rounds' spread (min .. max) beside it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ppo_cpp_amd

ROUNDS, REPS = 5, 40
SHAPES = ((18, 18, [256, 256]), (18, 6, [64, 64]))
HEADS = ("gaussian", "categorical")
ROWS = (1024, 4096)
E, T = 4096, 16


def timed(g, call, reps, all_classes=False):
    g.prof_enable(True)
    for _ in range(reps):
        call()
    p = g.prof_read()
    g.prof_enable(False)
    if all_classes:
        return sum(v[0] for v in p.values()) / reps * 1e3, sum(v[1] for v in p.values()) / reps
    ms, launches = p["policy_step"]
    assert launches, "nothing was booked under policy_step: %s" % p
    return ms / reps * 1e3, launches / reps


def row(name, xs):
    return "%-34s %8.2f   (%.2f .. %.2f)" % (name, np.median(xs), min(xs), max(xs))


def main():
    rng = np.random.RandomState(0)
    out = {}
    for O, A, hidden in SHAPES:
        for head in HEADS:
            g = ppo_cpp_amd.PPOHip(O, A, hidden, action_dist=head)
            g.init_orthogonal(0)
            obs = {n: rng.uniform(-1, 1, (n, O)).astype(np.float32) for n in ROWS + (E * T,)}
            acts = {n: g.step(obs[n])[0] for n in ROWS}
            g.rollout_alloc(E, T)
            g.collect_synthetic(3, 0.99, 0.95)                       # a finished rollout for rollout_evaluate
            calls = {}
            for n in ROWS:
                calls["step %d rows" % n] = (lambda n=n: g.step(obs[n]), REPS)
                calls["evaluate_actions %d rows" % n] = (lambda n=n: g.evaluate_actions(obs[n], acts[n]), REPS)
            calls["step %d rows" % (E * T)] = (lambda: g.step(obs[E * T]), 4)
            calls["rollout_evaluate %dx%d rows" % (E, T)] = (lambda: g.rollout_evaluate(), 4)
            calls["collect_synthetic %dx%d, all classes" % (E, T)] = (lambda: g.collect_synthetic(3, 0.99, 0.95), 4)
            for call, _ in calls.values():                             # warm-up of everything the timed rounds use (the rollout is finished from here on)
                for _ in range(3):
                    call()
            res = {k: [] for k in calls}
            launches = {}
            for _ in range(ROUNDS):
                for k, (call, reps) in calls.items():
                    us, nl = timed(g, call, reps, all_classes=k.startswith("collect"))
                    res[k].append(us); launches[k] = nl
            tag = "%d obs, %d %s, hidden %s" % (O, A, "actions" if head == "gaussian" else "categories", hidden)
            print(tag + "   (us of device time per call in the policy_step class -- collect_synthetic: all classes --, median of %d rounds, min .. max)" % ROUNDS)
            for k, xs in res.items():
                print("  " + row(k, xs) + "   launches per call %g" % launches[k])
            for n in ROWS:
                print("  evaluate_actions / step at %d rows: %.3f" % (n, np.median(res["evaluate_actions %d rows" % n]) / np.median(res["step %d rows" % n])))
            print("  rollout_evaluate / step at %d rows: %.3f" % (E * T, np.median(res["rollout_evaluate %dx%d rows" % (E, T)]) / np.median(res["step %d rows" % (E * T)])))
            print("  kernels:", {k: int(v) for k, v in g.kernel_counts().items() if v and "step" in k})
            out[tag] = {k: [float(x) for x in xs] for k, xs in res.items()}
            g.close()
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
