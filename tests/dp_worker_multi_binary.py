"""One rank of the two-process multi-binary data-parallel test (tests/test_multi_binary.py); not collected by pytest.
usage: dp_worker_multi_binary.py <rank> <world> <in.npz> <out.npz>      (PPO_RCCL_LIBRARY selects the collective library)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, fin, fout = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import ppo_cpp_amd
    d = np.load(fin)
    hidden = [int(x) for x in d["hidden"]]
    E, T, nmb, epochs, A = (int(d[k]) for k in ("E", "T", "nmb", "epochs", "A"))
    El = E // world
    sl = slice(rank * El, (rank + 1) * El)
    g = ppo_cpp_amd.PPOHip(18, A, hidden, device=0, action_dist="multi_binary")
    g.set_flat(d["theta"])
    g.dist_init(world, rank, d["uid"].tobytes())
    g.norm_init(El, 0.99)
    g.rollout_alloc(El, T)
    for f in ("obs", "actions", "values", "neglogp", "returns"):
        g.rollout_set(f, np.ascontiguousarray(d["ro_" + f][:, sl]))
    g.dist_global_shuffle(True)                                       # ONE permutation over the rows of all ranks, the same on every rank
    rows, mean = g.update(float(d["lr"]), float(d["cr"]), epochs, nmb, d["gperms"])
    out = {"rows": rows, "mean": mean, "theta": g.get_flat(0), "adam_m": g.get_flat(1), "adam_v": g.get_flat(2), "actions": g.rollout_get("actions")}
    g.close()
    np.savez(fout, **out)


if __name__ == "__main__":
    main()
