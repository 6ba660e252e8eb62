"""Device time of a PPO_BF16 handle's policy queries (ppo_set_bf16_queries: bf16_eval_kernel) against ppo_step on the same handle: ppo_prof_read's policy_step class
(events around staging, forward and epilogue), 256 observations, [1024,1024,1024], the Gaussian head (64 actions) and nvec = (16,) x 4, at 256 and 8192 rows.  One
process; per call kind 20 warm-up calls, then alternating rounds of 20 calls; prints median (min .. max over the rounds) in us per call and one JSON line.
usage: python tools/bf16_query_time.py [--rounds N]      (default 30; DESIGN.md section 5 holds a run)"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import ppo_cpp_amd

O, HIDDEN, CALLS = 256, [1024, 1024, 1024], 20
HEADS = {"gaussian": dict(act_dim=64), "mcat16x4": dict(act_dim=None, action_dist="multi_categorical", nvec=[16] * 4, bf16_head=True)}


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 30
    out = {}
    for head, kw in HEADS.items():
        kw = dict(kw)
        g = ppo_cpp_amd.PPOHip(O, kw.pop("act_dim"), HIDDEN, compute_dtype=1, **kw)
        g.init_orthogonal(0)
        g.set_bf16_queries(True)
        g.prof_enable(True)
        for n in (256, 8192):
            obs = np.random.RandomState(n).uniform(-1, 1, (n, O)).astype(np.float32)
            a = g.step(obs)[0]
            calls = {"step": lambda: g.step(obs), "evaluate_actions": lambda: g.evaluate_actions(obs, a), "action_probability": lambda: g.action_probability(obs)}
            for f in calls.values():
                for _ in range(CALLS):
                    f()
            per = {k: [] for k in calls}
            for _ in range(rounds):
                for k, f in calls.items():
                    ms0, c0 = g.prof_read()["policy_step"]
                    for _ in range(CALLS):
                        f()
                    ms1, c1 = g.prof_read()["policy_step"]
                    assert c1 - c0 == CALLS, (c0, c1)
                    per[k].append((ms1 - ms0) / CALLS * 1e3)
            out["%s n=%d" % (head, n)] = {k: [float(np.median(v)), float(np.min(v)), float(np.max(v))] for k, v in per.items()}
            print("%-9s %5d rows  " % (head, n) + "   ".join("%s %.1f (%.1f .. %.1f)" % ((k,) + tuple(v)) for k, v in out["%s n=%d" % (head, n)].items()), flush=True)
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
