"""Reference for action masks on the categorical policy head (invalid-action masking as sb3-contrib's MaskablePPO states it), built on
tests/categorical_ref.CatRef.

Forward pass in float64 NumPy with the formulas of include/ppo_hip.h (forbidden categories EXCLUDED: maximum, normaliser, both argmaxes and
the entropy run over the allowed set).  Loss and gradient by torch float64 autograd of sb3-contrib's expressions -- logits replaced by
where(mask, l, -1e8) before the softmax, the entropy summed over the allowed categories only -- not a restatement of the kernel's d logits.
With float64 and logits of order 1, exp(-1e8 - max) is exactly 0, so the two statements agree to the last bit of the reference.

Test infrastructure only: imported by tests/test_action_mask.py.
"""
import numpy as np

from tests.categorical_ref import CatRef


def masked_gumbel_argmax(logits, u, mask):
    """a = argmax_{j allowed} (l_j - log(-log u_j)); ties -> lowest index.  Also returns the perturbed logits with -inf on the forbidden ones."""
    with np.errstate(divide="ignore"):
        pert = logits - np.log(-np.log(u.astype(np.float64)))
    pert = np.where(mask != 0, pert, -np.inf)
    return np.argmax(pert, axis=1), pert


def masked_softmax_stats(logits, mask):
    """neglogp of every category (inf on forbidden ones), entropy over the allowed set and probabilities (0 on forbidden ones), float64"""
    ok = mask != 0
    m = np.where(ok, logits, -np.inf).max(axis=1, keepdims=True)
    a0 = logits - m
    e = np.where(ok, np.exp(np.where(ok, a0, 0.0)), 0.0)
    z = e.sum(axis=1, keepdims=True)
    p = e / z
    nlp_all = np.where(ok, np.log(z) - a0, np.inf)
    ent = np.where(ok, p * (np.log(z) - a0), 0.0).sum(axis=1)
    return nlp_all, ent, p


def random_masks(rng, n, A, special=True):
    """[n, A] float32: every category kept with probability 1/2, one allowed category forced per row; with `special`, the first rows (as many as
    fit) become: only category 0, only category A-1, only the categories >= 16 (A > 16), all allowed"""
    mask = (rng.uniform(size=(n, A)) < 0.5).astype(np.float32)
    mask[np.arange(n), rng.randint(0, A, n)] = 1.0
    if special:
        rows = [np.eye(A, dtype=np.float32)[0], np.eye(A, dtype=np.float32)[A - 1]]
        if A > 16:
            rows.append((np.arange(A) >= 16).astype(np.float32))
        rows.append(np.ones(A, np.float32))
        for i, r in enumerate(rows[:n]):
            mask[i] = r
    return mask


class MaskedCatRef(CatRef):
    def step(self, obs, u, mask=None):
        """(actions, values, neglogp, perturbed logits) under mask [n, A] (None: CatRef.step)"""
        if mask is None:
            return CatRef.step(self, obs, u)
        logits, v = self.forward(obs)
        a, pert = masked_gumbel_argmax(logits, u, mask)
        nlp_all, _, _ = masked_softmax_stats(logits, mask)
        return a, v, nlp_all[np.arange(len(a)), a], pert

    def act_deterministic(self, obs, mask):
        logits, _ = self.forward(obs)
        return np.argmax(np.where(mask != 0, logits, -np.inf), axis=1)

    def loss_grad(self, obs, actions, advs, returns, old_nlp, old_v, cr, mask=None):
        if mask is None:
            return CatRef.loss_grad(self, obs, actions, advs, returns, old_nlp, old_v, cr)
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
        # MaskableCategorical.apply_masking: logits = where(mask, logits, HUGE_NEG), then the ordinary categorical log-probability
        ok = torch.tensor(np.asarray(mask) != 0)
        ml = torch.where(ok, logits, torch.tensor(-1e8, dtype=d))
        logp = torch.log_softmax(ml, dim=1)
        nlp = -logp.gather(1, torch.tensor(np.asarray(actions).astype(np.int64)).reshape(-1, 1)).reshape(-1)
        # MaskableCategorical.entropy: p_log_p = logits * probs, where(mask, p_log_p, 0), -sum
        p_log_p = torch.where(ok, logp * torch.exp(logp), torch.tensor(0.0, dtype=d))
        entropy = (-p_log_p.sum(1)).mean()
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
        """CatRef.update with ro["masks"] [T, E, A] travelling with the rows (absent: unmasked)"""
        if "masks" not in ro:
            return CatRef.update(self, ro, perms, nminibatches, lr, cr)
        T, E = ro["values"].shape
        flat = {k: np.swapaxes(np.asarray(ro[k]), 0, 1).reshape((E * T,) + np.asarray(ro[k]).shape[2:]) for k in
                ("obs", "actions", "values", "neglogp", "returns", "masks")}
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
                losses, _ = self.train_step(lr, cr, flat["obs"][idx], flat["actions"][idx], adv, ret, flat["neglogp"][idx], val, flat["masks"][idx])
                rows.append(losses)
        rows = np.array(rows)
        return rows, rows.mean(axis=0)


def masked_learn_loop(env_step, env_reset, env_mask, ref, n_envs, n_steps, n_updates, lr, cr, gamma, lam, noptepochs, nminibatches, seed):
    """tests/categorical_ref.learn_loop with action masks: env_mask() -> [E, A] legality of the current observation, sampled under, kept with the row and
    trained under.  Returns (mean raw reward of every update's rollout, number of forbidden actions sent)."""
    rng = np.random.RandomState(seed)
    obs = env_reset()
    dones = np.zeros(n_envs)
    curve, forbidden = [], 0
    for _ in range(n_updates):
        ro = {k: [] for k in ("obs", "actions", "values", "neglogp", "dones", "rewards", "raw", "masks")}
        for t in range(n_steps):
            mask = env_mask()
            a, v, nlp, _ = ref.step(obs, rng.uniform(size=(n_envs, ref.A)), mask)
            forbidden += int((mask[np.arange(n_envs), a] == 0).sum())
            ro["obs"].append(obs); ro["actions"].append(a.astype(np.float64)); ro["values"].append(v); ro["neglogp"].append(nlp)
            ro["dones"].append(dones); ro["masks"].append(mask)
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
    return np.array(curve), forbidden
