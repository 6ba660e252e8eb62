"""One rank of the two-process truncation test (tests/test_truncation.py); not collected by pytest.
usage: dp_worker_truncation.py <rank> <world> <in.npz> <out.npz>      (PPO_RCCL_LIBRARY selects the collective library)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, fin, fout = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import ppo_cpp_amd
    from oracle import oracle as o
    d = np.load(fin)
    hidden = [int(x) for x in d["hidden"]]
    E, T, O, A, seed = (int(d[k]) for k in ("E", "T", "O", "A", "seed"))
    gamma, lam = float(d["gamma"]), float(d["lam"])
    El = E // world
    sl = slice(rank * El, (rank + 1) * El)
    step_dones, trunc, term_raw = d["step_dones"][:, sl], d["trunc"][:, sl], d["term_raw"][:, sl]
    g = ppo_cpp_amd.PPOHip(O, A, hidden, device=0)
    g.set_flat(d["theta"])
    g.seed(3)
    g.dist_init(world, rank, d["uid"].tobytes())
    g.norm_init(El)
    g.rollout_alloc(El, T)
    # this rank's columns of the job's environments (the seeded env is keyed by the global env id)
    g.rollout_reset(o.seeded_env_step(seed, 0, E, 0, O)[0][sl])
    for t in range(T):
        g.rollout_act(t)
        raw, rew, _ = o.seeded_env_step(seed, 0, E, t + 1, O)
        g.rollout_observe(t, raw[sl], rew[sl], step_dones[t])
        ids = np.nonzero(trunc[t])[0]
        if ids.size:
            g.rollout_mark_truncated(t, ids, term_raw[t, ids])
    g.rollout_finish(gamma, lam)
    out = {"returns": g.rollout_get("returns"), "values": g.rollout_get("values"), "tv": g.rollout_get("terminal_values")}
    out["scatter"] = np.int32(g.kernel_counts().get("tval_scatter_kernel", 0))
    g.update(3e-4, 0.2, 2, 4, None, seed=9 + (rank << 20), want_rows=False)
    out["theta"], out["adam_m"], out["adam_v"] = g.get_flat(0), g.get_flat(1), g.get_flat(2)
    out["obs_mean"], out["obs_var"], _ = g.norm_stats(0)
    g.close()
    np.savez(fout, **out)


if __name__ == "__main__":
    main()
