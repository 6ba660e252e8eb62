"""Reference for the multi-binary policy head (stable-baselines' BernoulliProbabilityDistribution on PPO2's two tanh towers).

Forward pass in float64 NumPy; loss and gradients by torch float64 autograd of the SMOOTH identity neglogp = sum_j softplus(l_j) - l_j z_j (z = the action for
neglogp, z = sigmoid(l) with the gradient flowing through it for the entropy) -- not a restatement of the kernel's hand-derived d logits, and not the literal
relu / abs expression, whose kinks autograd differentiates to 0 at a logit of exactly +-0 (include/ppo_hip.h says which one the library takes).  Everything that
does not depend on the head -- the parameter vector in the categorical tensor order (4L+4 tensors, no pi/logstd), the towers, clip_by_global_norm + Adam, the
minibatch update and the learning loop -- is CatRef's.

Test infrastructure only: imported by tests/test_multi_binary.py and tests/dp_worker_multi_binary.py.
"""
import numpy as np

from tests.categorical_ref import CatRef, learn_loop  # noqa: F401  (learn_loop: BernRef.step has CatRef.step's signature, so the loop is the same)


def bern_stats(logits):
    """(p, neglogp of the bit 1, neglogp of the bit 0, entropy per element) in float64, stable for any finite logit"""
    l = np.asarray(logits, np.float64)
    sp = np.log1p(np.exp(-np.abs(l)))                      # softplus(-|l|)
    nlp1 = sp + np.maximum(-l, 0.0)                        # softplus(-l) = -log sigmoid(l)
    nlp0 = sp + np.maximum(l, 0.0)                         # softplus(l)  = -log (1 - sigmoid(l))
    p = np.exp(-nlp1)
    ent = p * nlp1 + np.exp(-nlp0) * nlp0
    return p, nlp1, nlp0, ent


class BernRef(CatRef):
    learn_loop = staticmethod(learn_loop)

    def step(self, obs, u):
        """(x [n, A] of 0 / 1, values, neglogp, p) with explicit uniforms u [n, A]: x_j = u_j < sigmoid(l_j)"""
        logits, v = self.forward(obs)
        p, nlp1, nlp0, _ = bern_stats(logits)
        x = (np.asarray(u, np.float64) < p).astype(np.float64)
        return x, v, np.where(x > 0, nlp1, nlp0).sum(axis=1), p

    def act_deterministic(self, obs):
        """tf.round(sigmoid(l)) = (l > 0): a logit of +-0 gives 0"""
        return (self.forward(obs)[0] > 0).astype(np.float64)

    def neglogp_entropy(self, obs, x):
        logits, _ = self.forward(obs)
        _, nlp1, nlp0, ent = bern_stats(logits)
        return np.where(np.asarray(x) > 0, nlp1, nlp0).sum(axis=1), ent.sum(axis=1)

    def loss_grad(self, obs, actions, advs, returns, old_nlp, old_v, cr):
        import torch
        d = torch.float64
        th = torch.tensor(self.theta, dtype=d, requires_grad=True)

        def T(name):
            o, shape = self.offs[name]
            return th[o:o + int(np.prod(shape))].reshape(shape)

        x = torch.tensor(np.asarray(obs, np.float64))
        hp, hv = x, x
        for l in range(len(self.hidden)):
            hp = torch.tanh(hp @ T("pi_fc%d/w" % l) + T("pi_fc%d/b" % l))
            hv = torch.tanh(hv @ T("vf_fc%d/w" % l) + T("vf_fc%d/b" % l))
        logits = hp @ T("pi/w") + T("pi/b")
        v = (hv @ T("vf/w")).reshape(-1) + T("vf/b")[0]
        sp = torch.nn.functional.softplus
        z = torch.tensor(np.asarray(actions, np.float64).reshape(len(obs), self.A))
        nlp = (sp(logits) - logits * z).sum(1)
        entropy = (sp(logits) - logits * torch.sigmoid(logits)).sum(1).mean()
        R, vo = torch.tensor(np.asarray(returns, np.float64)), torch.tensor(np.asarray(old_v, np.float64))
        adv, onlp = torch.tensor(np.asarray(advs, np.float64)), torch.tensor(np.asarray(old_nlp, np.float64))
        # TF's Maximum / Minimum send the gradient to the first argument on a tie: torch.where does the same
        tmax = lambda p, q: torch.where(p >= q, p, q)
        tmin = lambda p, q: torch.where(p <= q, p, q)
        crt = torch.tensor(cr, dtype=d)
        vclip = vo + tmax(tmin(v - vo, crt), -crt)
        vf_loss = 0.5 * tmax((v - R) ** 2, (vclip - R) ** 2).mean()
        ratio = torch.exp(onlp - nlp)
        pg_loss = tmax(-adv * ratio, -adv * tmax(tmin(ratio, 1.0 + crt), 1.0 - crt)).mean()
        loss = pg_loss - self.ent * entropy + self.vfc * vf_loss
        loss.backward()
        with torch.no_grad():
            kl = 0.5 * ((nlp - onlp) ** 2).mean()
            cf = ((ratio - 1.0).abs() > cr).to(d).mean()
        losses = np.array([pg_loss.item(), vf_loss.item(), entropy.item(), kl.item(), cf.item()])
        return losses, th.grad.numpy().copy()

    def loss_value(self, theta, obs, actions, advs, returns, old_nlp, old_v, cr):
        """the scalar loss at `theta` in float64 NumPy (for central differences)"""
        keep = self.theta
        self.theta = np.asarray(theta, np.float64)
        try:
            logits, v = self.forward(obs)
        finally:
            self.theta = keep
        p, nlp1, nlp0, ent = bern_stats(logits)
        z = np.asarray(actions, np.float64).reshape(len(obs), self.A)
        nlp = np.where(z > 0, nlp1, nlp0).sum(axis=1)
        ratio = np.exp(np.asarray(old_nlp, np.float64) - nlp)
        adv = np.asarray(advs, np.float64)
        pg = np.maximum(-adv * ratio, -adv * np.clip(ratio, 1.0 - cr, 1.0 + cr)).mean()
        vo, R = np.asarray(old_v, np.float64), np.asarray(returns, np.float64)
        vclip = vo + np.clip(v - vo, -cr, cr)
        vf = 0.5 * np.maximum((v - R) ** 2, (vclip - R) ** 2).mean()
        return pg - self.ent * ent.sum(axis=1).mean() + self.vfc * vf


def emulate_f32(logits, u=None, x=None):
    """The stated form (include/ppo_hip.h) in float32 NumPy, element by element: returns (p, x, neglogp rows, entropy rows, p (1 - p))."""
    f = np.float32
    l = np.asarray(logits, f)
    e = np.exp(-np.abs(l), dtype=f)
    sp = np.log1p(e, dtype=f)
    q = (e / (f(1) + e)).astype(f)
    p = np.where(l >= 0, (f(1) / (f(1) + e)).astype(f), q).astype(f)
    if x is None:
        x = (np.asarray(u, f) < p).astype(f)
    nlp = (sp + np.where((x != 0) == (l > 0), f(0), np.abs(l))).astype(f)
    ent = (sp + np.abs(l) * q).astype(f)
    pq = (e / ((f(1) + e) * (f(1) + e))).astype(f)
    return p, x, nlp.sum(axis=1, dtype=f), ent.sum(axis=1, dtype=f), pq


# ---- host/env/env_mock.hpp's MultiBinaryTargetEnv in NumPy (the learning check's reference leg) ---------------------------------------------------------------
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _sym_unit(h):
    return np.float32(h >> 8) * np.float32(1.0 / 8388608.0) - np.float32(1.0)


class MultiBinaryTargetRef:
    """n_envs x MultiBinaryTargetEnv(seed, env_id = 0 .. n_envs - 1, obs_dim, n_bits, episode_len): the same observation streams, TargetEnv's hashed W,
    reward = the share of bits with x_j == ((W obs)_j > 0)."""

    def __init__(self, seed, n_envs, obs_dim, n_bits, episode_len=100):
        self.E, self.O, self.A, self.len = n_envs, obs_dim, n_bits, episode_len
        self.keys = [_splitmix64(((seed << 32) | e) & _M64) for e in range(n_envs)]
        wkey = _splitmix64(((seed << 32) | 0xffffffff) & _M64)
        self.W = np.array([[np.float32(0.5) * _sym_unit(_splitmix64(wkey ^ ((j << 32) | k)) >> 32) for k in range(obs_dim)] for j in range(n_bits)], np.float32)
        self.step_ = 0

    def obs_at(self, step):
        return np.array([[_sym_unit(_splitmix64(key ^ ((step << 32) | j)) >> 32) for j in range(self.O)] for key in self.keys], np.float32)

    def targets(self):
        return (self.obs_at(self.step_) @ self.W.T) > 0

    def reset(self):
        self.step_ = 0
        return self.obs_at(0)

    def step(self, actions):
        """(raw observations, raw rewards, dones)"""
        hits = ((np.asarray(actions) != 0) == self.targets()).sum(axis=1)
        self.step_ += 1
        done = np.full(self.E, 1.0 if self.step_ % self.len == 0 else 0.0, np.float32)
        return self.obs_at(self.step_), (hits / float(self.A)).astype(np.float32), done


def reference_curve(draw_seed, n_updates, n_envs=16, n_steps=64, hidden=(64, 64), n_bits=18, obs_dim=18, lr=2e-3, cr=0.2, gamma=0.99, lam=0.95, noptepochs=4,
                    nminibatches=4):
    """BernRef.learn_loop on MultiBinaryTargetRef(1234, ..) behind the oracle's EnvNormalize: the mean raw reward of every update's rollout.  The reference leg of
    tests/test_multi_binary.py's learning check; run `python -m tests.bernoulli_ref N` from the repository root to print the three seeds' curves."""
    from oracle import oracle as o
    env = MultiBinaryTargetRef(1234, n_envs, obs_dim, n_bits)
    nz = o.Normalizer(n_envs, obs_dim)
    ref = BernRef(obs_dim, n_bits, hidden)
    ref.init_random(draw_seed, pi_gain=0.01)

    def env_reset():
        return nz.obs(env.reset())

    def env_step(a):
        raw, rew, dones = env.step(a)
        return nz.obs(raw), nz.reward(rew, dones), dones, rew

    return learn_loop(env_step, env_reset, ref, n_envs, n_steps, n_updates, lr, cr, gamma, lam, noptepochs, nminibatches, draw_seed)


if __name__ == "__main__":
    import sys
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    for s in (0, 1, 2):
        c = reference_curve(s, N)
        print("seed %d first-15 %.4f last-15 %.4f rise %.4f" % (s, c[:15].mean(), c[-15:].mean(), c[-15:].mean() - c[:15].mean()), flush=True)
        print(" ".join("%.3f" % x for x in c), flush=True)
