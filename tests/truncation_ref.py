"""Arbiter for the value bootstrap at time-limit truncations (include/ppo_hip.h: ppo_gae_ex, ppo_rollout_mark_truncated).

The definition, in float64 NumPy: GAE exactly as Runner::set_returns runs it (nnt = 1 - done, so the lambda trace is cut at every episode
boundary) with the reward of a row replaced by rewards + gamma * tv, tv = V(terminal observation) on the rows a time limit cut and 0 elsewhere:

    delta_t = (rewards[t] + gamma tv[t]) + gamma V[t+1] (1 - done[t+1]) - V[t]

Also here: a float64 value tower read from a handle's tensors (any head, any width), EnvNormalize's observation scaling with given statistics,
the host-Env rollout of the seeded environment with caller-made dones and marks, and a small NumPy PPO loop on the unit-reward task for the
learning check.  The normaliser, the seeded env and the Gaussian policy come from oracle/ (imported, never edited).

Test infrastructure only: imported by tests/test_truncation.py.
"""
import numpy as np


def gae_truncated(rewards, values, dones, last_values, last_dones, tv, gamma, lam):
    """[T, E] time-major, float64.  dones[t] = the done that arrived WITH observation t (raised by step t-1); last_dones = raised by step T-1."""
    rw, va, dn, tv = [np.asarray(x, np.float64) for x in (rewards, values, dones, tv)]
    T, E = rw.shape
    out = np.empty((T, E), np.float64)
    last = np.zeros(E)
    nv = np.asarray(last_values, np.float64).reshape(E)
    nnt = 1.0 - np.asarray(last_dones, np.float64).reshape(E)
    for t in range(T - 1, -1, -1):
        delta = (rw[t] + gamma * tv[t]) + gamma * nv * nnt - va[t]
        last = delta + gamma * lam * nnt * last
        out[t] = last + va[t]
        nv = va[t]
        nnt = 1.0 - dn[t]
    return out


def value_tower(g, obs):
    """V(obs) in float64 from the handle's own tensors (vf_fc*/w, vf_fc*/b, vf/w, vf/b): the same for a Gaussian, a categorical and a bf16 handle"""
    h = np.asarray(obs, np.float64)
    for l in range(len(g.hidden)):
        h = np.tanh(h @ g.get_tensor("vf_fc%d/w" % l).astype(np.float64) + g.get_tensor("vf_fc%d/b" % l).astype(np.float64))
    return (h @ g.get_tensor("vf/w").astype(np.float64)).reshape(-1) + float(g.get_tensor("vf/b")[0])


def scale_obs(raw, mean, var, clip=10.0, eps=1e-8):
    """EnvNormalize's observation scaling (env_normalize.hpp:100-104) with GIVEN statistics, which stay as they are"""
    x = (np.asarray(raw, np.float64) - np.asarray(mean, np.float64)) / np.sqrt(np.asarray(var, np.float64) + eps)
    return np.clip(x, -clip, clip)


def make_marks(rng, T, E, p_done=0.03, force=((0, 0), (-1, 0))):
    """step_dones [T, E]: the done RAISED BY step t; trunc [T, E]: about half of them are time-limit truncations.  `force`: (t, e) pairs that are
    truncations for sure (the first and the last step by default)."""
    step_dones = (rng.uniform(size=(T, E)) < p_done).astype(np.float32)
    trunc = (step_dones > 0) & (rng.uniform(size=(T, E)) < 0.5)
    for t, e in force:
        step_dones[t, e] = 1.0
        trunc[t, e] = True
    return step_dones, trunc


def shift_dones(step_dones):
    """(dones [T, E] as the rollout stores them -- row t holds the done raised by step t-1, row 0 zeros -- and last_dones [E])"""
    d = np.zeros_like(step_dones)
    d[1:] = step_dones[:-1]
    return d, step_dones[-1].copy()


def host_rollout(g, seed, E, T, step_dones, trunc, term_raw, gamma, lam, noise=None, mark=True):
    """The host-Env loop (reset / act / observe / mark_truncated / finish) over the seeded env, whose dones are replaced by step_dones.
    term_raw [T, E, O]: raw terminal observations (used where trunc).  noise: [T, E, A] explicit draws or None (on-device generator)."""
    from oracle import oracle as o
    O = g.O
    raw, _, _ = o.seeded_env_step(seed, 0, E, 0, O)
    g.rollout_reset(raw)
    for t in range(T):
        g.rollout_act(t, None if noise is None else noise[t])
        raw, rew, _ = o.seeded_env_step(seed, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, step_dones[t])
        ids = np.nonzero(trunc[t])[0]
        if mark and ids.size:
            g.rollout_mark_truncated(t, ids, term_raw[t, ids])
    g.rollout_finish(gamma, lam)


def ref_rollout(g, seed, E, T, step_dones, trunc, term_raw, gamma, lam, norm_gamma=0.99):
    """What host_rollout must leave behind, from the handle's weights: obs (fp32 oracle normaliser), rewards, values and terminal values (float64
    tower), returns (float64 GAE above).  The seeded env ignores the actions, so nothing here depends on the policy head."""
    from oracle import oracle as o
    O = g.O
    nz = o.Normalizer(E, O, gamma=norm_gamma)
    raw, _, _ = o.seeded_env_step(seed, 0, E, 0, O)
    obs = nz.obs(raw)
    ro = {k: [] for k in ("obs", "values", "rewards")}
    for t in range(T):
        ro["obs"].append(obs)
        ro["values"].append(value_tower(g, obs))
        raw, rew, _ = o.seeded_env_step(seed, 0, E, t + 1, O)
        obs = nz.obs(raw)
        ro["rewards"].append(nz.reward(rew, step_dones[t]))
    ro = {k: np.array(x) for k, x in ro.items()}
    last_v = value_tower(g, obs)
    # the terminal observations: the statistics as they stand at the finish, never updated by them
    tv = np.zeros((T, E))
    tt, ee = np.nonzero(trunc)
    if tt.size:
        tv[tt, ee] = value_tower(g, scale_obs(term_raw[tt, ee], nz.obs_rms.mean, nz.obs_rms.var))
    dones, last_dones = shift_dones(step_dones)
    ro["dones"], ro["terminal_values"] = dones, tv
    ro["returns"] = gae_truncated(ro["rewards"], ro["values"], dones, last_v, last_dones, tv, gamma, lam)
    ro["obs_rms"] = (nz.obs_rms.mean.copy(), nz.obs_rms.var.copy(), nz.obs_rms.count)
    return ro


def learn_unit_reward(seed, n_updates, bootstrap, probe_raw, E=16, T=32, L=20, gamma=0.9, lam=0.95, lr=1e-3, cr=0.2, epochs=4, nmb=4, O=18, A=18,
                      hidden=(64, 64), env_seed=1234):
    """PPO2 on E x TimeLimit(UnitRewardEnv, L) (host/env/env_mock.hpp: SeededEnvMock's observation stream, which a reset moves one draw on, reward 1,
    episodes end by the time limit only) with the oracle's Gaussian policy, EnvNormalize (norm_reward off) and update.  bootstrap: the rule above; otherwise
    every done is terminal.  Returns the mean critic value over probe_raw after every update [n_updates]."""
    from oracle import oracle as o
    rng = np.random.RandomState(seed)
    orc = o.Oracle(O, A, list(hidden))
    orc.init_orthogonal(seed)
    nz = o.Normalizer(E, O, gamma=gamma)
    env_obs = lambda k: o.seeded_env_step(env_seed, 0, E, k, O)[0]
    k, n = 1, 0                                                     # k: position in the stream (the pool's one reset was draw 1), n: steps of the episode
    obs = nz.obs(env_obs(k))
    dones = np.zeros(E, np.float32)
    curve = []
    for _ in range(n_updates):
        ro = {f: [] for f in ("obs", "actions", "values", "neglogp", "dones")}
        term = []                                                   # (t, raw terminal observation [E, O]): all envs run in step
        for t in range(T):
            a, v, nlp = orc.step(obs, rng.normal(size=(E, A)))
            for f, x in (("obs", obs), ("actions", a), ("values", v), ("neglogp", nlp), ("dones", dones)):
                ro[f].append(x)
            k += 1
            n += 1
            raw = env_obs(k)
            dones = np.zeros(E, np.float32)
            if n >= L:
                term.append((t, raw))
                k += 1
                n = 0
                raw = env_obs(k)
                dones = np.ones(E, np.float32)
            obs = nz.obs(raw)
        ro = {f: np.array(x) for f, x in ro.items()}
        tv = np.zeros((T, E))
        if bootstrap:
            for t, raw in term:
                tv[t] = orc.forward(scale_obs(raw, nz.obs_rms.mean, nz.obs_rms.var).astype(np.float32))[1]
        _, last_v = orc.forward(obs)
        ro["returns"] = gae_truncated(np.ones((T, E)), ro["values"], ro["dones"], last_v, dones, tv, gamma, lam).astype(np.float32)
        perms = np.stack([rng.permutation(E * T).astype(np.int32) for _ in range(epochs)])
        orc.update(ro, perms, nmb, lr, cr)
        curve.append(float(orc.forward(scale_obs(probe_raw, nz.obs_rms.mean, nz.obs_rms.var).astype(np.float32))[1].mean()))
    return np.array(curve)


def probe_batch(n=64, O=18, seed=5):
    """the fixed probe batch of the learning check: raw observations from the environment's own distribution, U(-1, 1)^O"""
    return np.random.RandomState(seed).uniform(-1, 1, (n, O)).astype(np.float32)
