"""One rank of the two-process draw test (tests/test_counter_draws.py); not collected by pytest.
usage: dp_worker_draws.py <rank> <world> <in.npz> <out.npz>      (PPO_RCCL_LIBRARY selects the collective library)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, fin, fout = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import ppo_cpp_amd
    from tests.test_counter_draws import zero_head
    d = np.load(fin)
    E, T, nmb, epochs, key, seed, shuffle_seed = (int(d[k]) for k in ("E", "T", "nmb", "epochs", "key", "seed", "shuffle_seed"))
    g = zero_head(ppo_cpp_amd.PPOHip(18, 18, [64, 64], device=0))
    g.seed(seed)
    g.dist_init(world, rank, d["uid"].tobytes())
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(key, float(d["gamma"]), float(d["lam"]), None, env0=rank * E, step0=0, first=True)
    out = {"actions": g.rollout_get("actions"), "neglogp": g.rollout_get("neglogp"), "comm_nranks": np.int32(g.dist_info()["comm_nranks"])}
    obs = np.random.RandomState(1).uniform(-1, 1, (E, 18)).astype(np.float32)
    out["step_a"], _, out["step_nlp"] = g.step(obs)
    g.dist_global_shuffle(True)
    g.update(float(d["lr"]), float(d["cr"]), epochs, nmb, None, seed=shuffle_seed, want_rows=False)
    out["gidx"] = g.debug_buffer("gidx")[:E * T].astype(np.int64)
    g.close()
    np.savez(fout, **out)


if __name__ == "__main__":
    main()
