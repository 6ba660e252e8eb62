"""Reference for the multi-categorical policy head (stable-baselines' MultiCategoricalProbabilityDistribution on PPO2's two tanh towers): K independent
categorical components over one logits vector of width A = sum(nvec), masks by exclusion per component.  Built on tests/masked_categorical_ref.MaskedCatRef
(and through it tests/categorical_ref.CatRef): parameters, forward pass, clip + Adam and the update loop are theirs.

Forward pass in float64 NumPy.  Loss and gradient by torch float64 autograd of the stable-baselines expressions -- per-component log_softmax against
one_hot(a_k), per-component entropy, both summed over the components in component order -- not a restatement of the kernel's hand-derived d logits.  Under a
mask the component's logits are replaced by where(mask, l, -1e8) before the softmax and the entropy runs over the allowed categories (sb3-contrib's
MaskableMultiCategorical), which in float64 with logits of order 1 is exclusion to the last bit.

Actions are [n, K] arrays, column k the index within component k.  With nvec = [A] every expression is CatRef's own, in the same order.

Test infrastructure only: imported by tests/test_multi_discrete.py.
"""
import numpy as np

from tests.categorical_ref import CatRef, gumbel_argmax, softmax_stats
from tests.masked_categorical_ref import MaskedCatRef, masked_gumbel_argmax, masked_softmax_stats


def offsets(nvec):
    return np.concatenate([[0], np.cumsum(nvec)]).astype(np.int64)


def random_masks(rng, n, nvec, special=True):
    """[n, A] float32: every category kept with probability 1/2, one allowed category forced per (row, component); with `special`, the first rows become:
    only the first category of every component, only the last one, all allowed"""
    off = offsets(nvec)
    A = int(off[-1])
    mask = (rng.uniform(size=(n, A)) < 0.5).astype(np.float32)
    for k, nk in enumerate(nvec):
        mask[np.arange(n), off[k] + rng.randint(0, nk, n)] = 1.0
    if special:
        first, last = np.zeros(A, np.float32), np.zeros(A, np.float32)
        first[off[:-1]] = 1.0
        last[off[1:] - 1] = 1.0
        for i, r in enumerate([first, last, np.ones(A, np.float32)][:n]):
            mask[i] = r
    return mask


class MultiCatRef(MaskedCatRef):
    def __init__(self, O, nvec, hidden, **kw):
        self.nvec = [int(x) for x in nvec]
        self.off = offsets(self.nvec)
        self.K = len(self.nvec)
        MaskedCatRef.__init__(self, O, int(self.off[-1]), hidden, **kw)

    def comp(self, x, k):
        return x[:, self.off[k]:self.off[k + 1]]

    # ---- forward (float64 NumPy) ----------------------------------------------------------------------------------------
    def stats(self, logits, mask=None):
        """per component: (neglogp of every category, entropy, probabilities)"""
        if mask is None:
            return [softmax_stats(self.comp(logits, k)) for k in range(self.K)]
        return [masked_softmax_stats(self.comp(logits, k), self.comp(mask, k)) for k in range(self.K)]

    def neglogp_of(self, logits, actions, mask=None):
        """row totals of the components' neglogp for actions [n, K], added in component order"""
        a = np.asarray(actions).astype(np.int64).reshape(len(logits), self.K)
        tot = None
        for k, (nlp_all, _, _) in enumerate(self.stats(logits, mask)):
            x = nlp_all[np.arange(len(a)), a[:, k]]
            tot = x if tot is None else tot + x
        return tot

    def entropy_of(self, logits, mask=None):
        tot = None
        for _, ent, _ in self.stats(logits, mask):
            tot = ent if tot is None else tot + ent
        return tot

    def step(self, obs, u, mask=None):
        """(actions [n, K], values, neglogp, perturbed logits [n, A]: -inf on forbidden ones) with explicit uniforms u [n, A]"""
        logits, v = self.forward(obs)
        acts, perts = [], []
        for k in range(self.K):
            if mask is None:
                a, pert = gumbel_argmax(self.comp(logits, k), self.comp(u, k))
            else:
                a, pert = masked_gumbel_argmax(self.comp(logits, k), self.comp(u, k), self.comp(mask, k))
            acts.append(a); perts.append(pert)
        a = np.stack(acts, axis=1)
        return a, v, self.neglogp_of(logits, a, mask), np.concatenate(perts, axis=1)

    def act_deterministic(self, obs, mask=None):
        logits, _ = self.forward(obs)
        if mask is not None:
            logits = np.where(mask != 0, logits, -np.inf)
        return np.stack([np.argmax(self.comp(logits, k), axis=1) for k in range(self.K)], axis=1)

    def top2_gap(self, x):
        """[n, K]: distance of the two best entries of every component of x [n, A] (perturbed or plain logits; -inf = forbidden)"""
        gaps = []
        for k in range(self.K):
            s = np.sort(self.comp(x, k), axis=1)[:, -2:]
            with np.errstate(invalid="ignore"):
                gaps.append(np.where(np.isinf(s[:, 0]), np.inf, s[:, 1] - s[:, 0]))
        return np.stack(gaps, axis=1)

    # ---- loss and gradient (torch float64 autograd) ---------------------------------------------------------------------
    def loss_grad(self, obs, actions, advs, returns, old_nlp, old_v, cr, mask=None):
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
        acts = np.asarray(actions).astype(np.int64).reshape(len(x), self.K)
        nlp, ent_rows = None, None
        for k in range(self.K):
            lk = logits[:, self.off[k]:self.off[k + 1]]
            ak = torch.tensor(acts[:, k])
            if mask is None:
                # MultiCategoricalProbabilityDistribution.neglogp / .entropy: the categorical expressions per component, tf.add_n over the components
                onehot = torch.nn.functional.one_hot(ak, self.nvec[k]).to(d)
                nk = -(onehot * torch.log_softmax(lk, dim=1)).sum(1)
                a0 = lk - lk.max(dim=1, keepdim=True).values
                z0 = torch.exp(a0).sum(1, keepdim=True)
                p0 = torch.exp(a0) / z0
                ek = (p0 * (torch.log(z0) - a0)).sum(1)
            else:
                ok = torch.tensor(np.asarray(mask)[:, self.off[k]:self.off[k + 1]] != 0)
                logp = torch.log_softmax(torch.where(ok, lk, torch.tensor(-1e8, dtype=d)), dim=1)
                nk = -logp.gather(1, ak.reshape(-1, 1)).reshape(-1)
                ek = -torch.where(ok, logp * torch.exp(logp), torch.tensor(0.0, dtype=d)).sum(1)
            nlp = nk if nlp is None else nlp + nk
            ent_rows = ek if ent_rows is None else ent_rows + ek
        entropy = ent_rows.mean()
        R, vo = torch.tensor(np.asarray(returns, np.float64)), torch.tensor(np.asarray(old_v, np.float64))
        adv, onlp = torch.tensor(np.asarray(advs, np.float64)), torch.tensor(np.asarray(old_nlp, np.float64))
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

    def train_step(self, lr, cr, obs, actions, advs, returns, old_nlp, old_v, mask=None):
        losses, grad = self.loss_grad(obs, actions, advs, returns, old_nlp, old_v, cr, mask)
        self.clip_adam(grad, lr)
        return losses, grad

    def update(self, ro, perms, nminibatches, lr, cr):
        """MaskedCatRef.update's loop (ro["masks"] [T, E, A] optional; ro["actions"] [T, E, K]) through this class's train_step"""
        T, E = ro["values"].shape
        keys = ("obs", "actions", "values", "neglogp", "returns") + (("masks",) if "masks" in ro else ())
        flat = {k: np.swapaxes(np.asarray(ro[k]), 0, 1).reshape((E * T,) + np.asarray(ro[k]).shape[2:]) for k in keys}
        B = E * T
        M = B // nminibatches
        rows = []
        for perm in perms:
            inv = np.empty(B, np.int64)
            inv[np.asarray(perm)] = np.arange(B)
            for k in range(nminibatches):
                idx = inv[k * M:(k + 1) * M]
                ret, val = flat["returns"][idx], flat["values"][idx]
                adv = ret.astype(np.float32) - val.astype(np.float32)
                adv = (adv - adv.mean(dtype=np.float64)) / (adv.std(dtype=np.float64) + 1e-8)
                losses, _ = self.train_step(lr, cr, flat["obs"][idx], flat["actions"][idx], adv, ret, flat["neglogp"][idx], val,
                                            flat["masks"][idx] if "masks" in flat else None)
                rows.append(losses)
        rows = np.array(rows)
        return rows, rows.mean(axis=0)


def learn_loop(env_step, env_reset, ref, n_envs, n_steps, n_updates, lr, cr, gamma, lam, noptepochs, nminibatches, seed):
    """tests/categorical_ref.learn_loop with [E, K] actions: env_reset() -> obs [E, O]; env_step(actions [E, K]) -> (obs, rewards, dones, raw rewards).
    Returns the mean raw reward of every update's rollout."""
    rng = np.random.RandomState(seed)
    obs = env_reset()
    dones = np.zeros(n_envs)
    curve = []
    for _ in range(n_updates):
        ro = {k: [] for k in ("obs", "actions", "values", "neglogp", "dones", "rewards", "raw")}
        for t in range(n_steps):
            a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n_envs, ref.A)))
            ro["obs"].append(obs); ro["actions"].append(a.astype(np.float64)); ro["values"].append(v); ro["neglogp"].append(nlp)
            ro["dones"].append(dones)
            obs, rew, dones, raw = env_step(a)
            ro["rewards"].append(rew); ro["raw"].append(raw)
        ro = {k: np.array(x) for k, x in ro.items()}
        _, last_v = ref.forward(obs)
        adv = np.zeros(n_envs); ret = np.empty((n_steps, n_envs))
        for t in range(n_steps - 1, -1, -1):
            nonterm = 1.0 - (dones if t == n_steps - 1 else ro["dones"][t + 1])
            nextv = last_v if t == n_steps - 1 else ro["values"][t + 1]
            delta = ro["rewards"][t] + gamma * nextv * nonterm - ro["values"][t]
            adv = delta + gamma * lam * nonterm * adv
            ret[t] = adv + ro["values"][t]
        ro["returns"] = ret
        B = n_envs * n_steps
        perms = np.stack([rng.permutation(B) for _ in range(noptepochs)])
        ref.update(ro, perms, nminibatches, lr, cr)
        curve.append(ro["raw"].mean())
    return np.array(curve)


# ---- host/env/env_mock.hpp's MultiDiscreteTargetEnv in NumPy (the learning check's reference leg) -------------------------------------------------------------
_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _sym_unit(h):
    return np.float32(h >> 8) * np.float32(1.0 / 8388608.0) - np.float32(1.0)


class MultiDiscreteTargetRef:
    """n_envs x MultiDiscreteTargetEnv(seed, env_id = 0 .. n_envs - 1, obs_dim, nvec, episode_len), unmasked: the same observation streams, the same hashed W_k
    (component k under key splitmix64(wkey ^ ((k + 1) << 48))), reward = fraction of components whose action is argmax_j (W_k obs)_j."""

    def __init__(self, seed, n_envs, obs_dim, nvec, episode_len=100):
        self.E, self.O, self.nvec, self.len = n_envs, obs_dim, list(nvec), episode_len
        self.keys = [_splitmix64(((seed << 32) | e) & _M64) for e in range(n_envs)]
        wkey = _splitmix64(((seed << 32) | 0xffffffff) & _M64)
        self.W = []
        for k, nk in enumerate(self.nvec):
            ck = _splitmix64(wkey ^ ((k + 1) << 48))
            self.W.append(np.array([[np.float32(0.5) * _sym_unit(_splitmix64(ck ^ ((j << 32) | i)) >> 32) for i in range(obs_dim)] for j in range(nk)], np.float32))
        self.step_ = 0

    def obs_at(self, step):
        return np.array([[_sym_unit(_splitmix64(key ^ ((step << 32) | j)) >> 32) for j in range(self.O)] for key in self.keys], np.float32)

    def targets(self):
        cur = self.obs_at(self.step_)
        return np.stack([np.argmax(cur @ w.T, axis=1) for w in self.W], axis=1)

    def reset(self):
        self.step_ = 0
        return self.obs_at(0)

    def step(self, actions):
        """(raw observations, raw rewards, dones)"""
        hits = (np.asarray(actions).astype(np.int64) == self.targets()).sum(axis=1)
        self.step_ += 1
        done = np.full(self.E, 1.0 if self.step_ % self.len == 0 else 0.0, np.float32)
        return self.obs_at(self.step_), (hits / float(len(self.nvec))).astype(np.float32), done
