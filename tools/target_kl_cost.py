"""What target-KL early stopping (ppo_set_target_kl) costs per train step of ppo_update on ONE GPU, by replaying the update's graph:
   off   the setting off: the handle's own forms (deferred Adam / resident epochs on the narrow reference shapes)
   on    a limit that never triggers (target_kl = 1e30): the forms that end every step in adam_kernel, the gate's loads and the counter
   skip  a limit that step 0 exceeds: one computed step, then every launch of the remaining steps returns at entry (the epoch preparation still runs)
Three handles per configuration, timed in alternating rounds; median (min - max) over the rounds.    usage: python tools/target_kl_cost.py [cfg2 cfg4 cfg3 ...]"""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench, ppo_cpp_amd

ROUNDS, UPDATES = 3, 20
for name in (sys.argv[1:] or ["cfg2", "cfg4", "cfg3"]):
    cfg = bench.CONFIGS[name]
    E, T, nmb, ep = cfg["n_envs"], cfg["n_steps"], cfg["nminibatches"], cfg["noptepochs"]
    steps = ep * nmb
    handles = {}
    for mode in ("off", "on", "skip"):
        g = ppo_cpp_amd.PPOHip(cfg["obs"], cfg["act"], cfg["hidden"])
        g.init_orthogonal(0)
        g.norm_init(E, bench.GAMMA); g.rollout_alloc(E, T)
        g.collect_synthetic(1234, bench.GAMMA, bench.LAM, None, env0=0, step0=0, first=True)
        g.update(bench.LR, bench.CR, ep, nmb, None, seed=0, want_rows=False)          # moves the policy off the rollout's: approxkl > 0 from here on
        g.set_target_kl({"off": 0.0, "on": 1e30, "skip": 1e-12}[mode])
        for i in range(2):
            g.update(bench.LR, bench.CR, ep, nmb, None, seed=1 + i, want_rows=False)
        want = (0, steps) if mode == "skip" else (steps, steps)
        assert g.update_applied() == want, (mode, g.update_applied())
        handles[mode] = g
    per_step = {m: [] for m in handles}
    for r in range(ROUNDS):
        for mode, g in handles.items():
            g.sync(); t0 = time.perf_counter()
            for i in range(UPDATES):
                g.update(bench.LR, bench.CR, ep, nmb, None, seed=10 + i, want_rows=False)
            g.sync()
            per_step[mode].append(1e6 * (time.perf_counter() - t0) / UPDATES / steps)
    kc = handles["on"].kernel_counts()
    for mode, v in per_step.items():
        print("%s %-4s %.2f us per train step, median of %d rounds x %d updates x %d steps (%.2f - %.2f)" %
              (name, mode, statistics.median(v), ROUNDS, UPDATES, steps, min(v), max(v)), flush=True)
    print("%s on: narrow_epoch_kernel %d" % (name, kc.get("narrow_epoch_kernel", 0)), flush=True)
    for g in handles.values():
        g.close()
