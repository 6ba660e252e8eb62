"""Reference for the categorical policy head (stable-baselines' CategoricalProbabilityDistribution on PPO2's two tanh towers).

Forward pass in float64 NumPy; loss and gradients by torch float64 autograd of the stable-baselines expressions (not a restatement of the
kernel's hand-derived d logits); clip_by_global_norm + Adam as TF applies them.  Parameters are kept as a dense flat vector in the library's
categorical tensor order (4L+4 tensors, no pi/logstd), so that a handle's get_flat / set_flat compare with it directly.

Test infrastructure only: imported by tests/test_discrete_policy.py.
"""
import numpy as np

G_ENT_COEF = 0.0007160293171182275     # the graph-baked defaults (ppo_config_default)
G_VF_COEF, G_MAX_GRAD_NORM = 0.5, 0.5
G_BETA1, G_BETA2, G_EPS = 0.8999999761581421, 0.9990000128746033, 9.999999747378752e-06


def tensor_specs(O, A, hidden):
    """(name, shape) in TF trainable-variable order without the Gaussian's pi/logstd"""
    specs = []
    for l, h in enumerate(hidden):
        inp = hidden[l - 1] if l else O
        specs += [("pi_fc%d/w" % l, (inp, h)), ("pi_fc%d/b" % l, (h,)), ("vf_fc%d/w" % l, (inp, h)), ("vf_fc%d/b" % l, (h,))]
    H = hidden[-1]
    return specs + [("vf/w", (H, 1)), ("vf/b", (1,)), ("pi/w", (H, A)), ("pi/b", (A,))]


def gumbel_argmax(logits, u):
    """a = argmax_j (l_j - log(-log u_j)); ties -> lowest index (np.argmax, like tf.argmax).  Also returns the perturbed logits."""
    with np.errstate(divide="ignore"):
        pert = logits - np.log(-np.log(u.astype(np.float64)))
    return np.argmax(pert, axis=1), pert


def softmax_stats(logits):
    """neglogp of every category, entropy and probabilities (stable-baselines' expressions) in float64"""
    m = logits.max(axis=1, keepdims=True)
    a0 = logits - m
    z = np.exp(a0).sum(axis=1, keepdims=True)
    p = np.exp(a0) / z
    nlp_all = np.log(z) - a0
    ent = (p * (np.log(z) - a0)).sum(axis=1)
    return nlp_all, ent, p


class CatRef:
    def __init__(self, O, A, hidden, ent_coef=G_ENT_COEF, vf_coef=G_VF_COEF, max_grad_norm=G_MAX_GRAD_NORM,
                 beta1=G_BETA1, beta2=G_BETA2, eps=G_EPS):
        self.O, self.A, self.hidden = O, A, list(hidden)
        self.specs = tensor_specs(O, A, hidden)
        self.offs = {}
        o = 0
        for name, shape in self.specs:
            self.offs[name] = (o, shape)
            o += int(np.prod(shape))
        self.P = o
        self.theta = np.zeros(o, np.float64)
        self.m = np.zeros(o, np.float64)
        self.v = np.zeros(o, np.float64)
        self.ent, self.vfc, self.maxn = ent_coef, vf_coef, max_grad_norm
        self.b1, self.b2, self.eps = beta1, beta2, eps
        self.pow = [beta1, beta2]

    def t(self, name, vec=None):
        o, shape = self.offs[name]
        vec = self.theta if vec is None else vec
        return vec[o:o + int(np.prod(shape))].reshape(shape)

    def init_random(self, seed, pi_gain=1.0):
        """orthogonal weights (gain sqrt 2 hidden, pi_gain head, 1 value head), small random biases: logits far from uniform"""
        rng = np.random.RandomState(seed)
        for name, shape in self.specs:
            if name.endswith("/w"):
                q, _ = np.linalg.qr(rng.normal(size=(max(shape), min(shape))))
                w = q if shape[0] >= shape[1] else q.T
                gain = pi_gain if name == "pi/w" else 1.0 if name == "vf/w" else np.sqrt(2.0)
                self.t(name)[:] = gain * w
            else:
                self.t(name)[:] = rng.uniform(-0.2, 0.2, shape)
        self.theta[:] = self.theta.astype(np.float32)          # the handle holds fp32

    # ---- forward (float64 NumPy) ----------------------------------------------------------------------------------------
    def forward(self, obs):
        x = np.asarray(obs, np.float64)
        hp, hv = x, x
        for l in range(len(self.hidden)):
            hp = np.tanh(hp @ self.t("pi_fc%d/w" % l) + self.t("pi_fc%d/b" % l))
            hv = np.tanh(hv @ self.t("vf_fc%d/w" % l) + self.t("vf_fc%d/b" % l))
        return hp @ self.t("pi/w") + self.t("pi/b"), (hv @ self.t("vf/w")).reshape(-1) + self.t("vf/b")[0]

    def step(self, obs, u):
        """(actions, values, neglogp, perturbed logits) of MlpPolicy::step with explicit uniforms u [n, A]"""
        logits, v = self.forward(obs)
        a, pert = gumbel_argmax(logits, u)
        nlp_all, _, _ = softmax_stats(logits)
        return a, v, nlp_all[np.arange(len(a)), a], pert

    # ---- loss and gradient (torch float64 autograd) ---------------------------------------------------------------------
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
        # CategoricalProbabilityDistribution.neglogp: softmax_cross_entropy_with_logits_v2(labels=one_hot(a))
        onehot = torch.nn.functional.one_hot(torch.tensor(np.asarray(actions).astype(np.int64)), self.A).to(d)
        nlp = -(onehot * torch.log_softmax(logits, dim=1)).sum(1)
        # .entropy(): a0 = l - max, p0 = exp(a0) / z0, sum p0 (log z0 - a0)
        a0 = logits - logits.max(dim=1, keepdim=True).values
        z0 = torch.exp(a0).sum(1, keepdim=True)
        p0 = torch.exp(a0) / z0
        entropy = (p0 * (torch.log(z0) - a0)).sum(1).mean()
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

    def clip_adam(self, grad, lr):
        norm = np.sqrt(np.dot(grad, grad))
        g = grad * (self.maxn * min(1.0 / norm, 1.0 / self.maxn))
        b1p, b2p = self.pow
        alpha = lr * np.sqrt(1.0 - b2p) / (1.0 - b1p)
        self.m += (g - self.m) * (1.0 - self.b1)
        self.v += (g * g - self.v) * (1.0 - self.b2)
        self.theta -= alpha * self.m / (np.sqrt(self.v) + self.eps)
        self.pow = [b1p * self.b1, b2p * self.b2]
        return norm

    def train_step(self, lr, cr, obs, actions, advs, returns, old_nlp, old_v):
        losses, grad = self.loss_grad(obs, actions, advs, returns, old_nlp, old_v, cr)
        self.clip_adam(grad, lr)
        return losses, grad

    def update(self, ro, perms, nminibatches, lr, cr):
        """ppo_update on a [T, E] rollout dict: perms[ep][i] = destination of env-major row i = e * T + t; per-minibatch advantage
        normalisation (ppo2.hpp:401-406); returns (loss rows, their column means)"""
        T, E = ro["values"].shape
        flat = {k: np.swapaxes(np.asarray(ro[k]), 0, 1).reshape((E * T,) + np.asarray(ro[k]).shape[2:]) for k in
                ("obs", "actions", "values", "neglogp", "returns")}
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
                losses, _ = self.train_step(lr, cr, flat["obs"][idx], flat["actions"][idx], adv, ret, flat["neglogp"][idx], val)
                rows.append(losses)
        rows = np.array(rows)
        return rows, rows.mean(axis=0)


def learn_loop(env_step, env_reset, ref, n_envs, n_steps, n_updates, lr, cr, gamma, lam, noptepochs, nminibatches, seed):
    """A plain NumPy categorical PPO loop over a vectorised env (the caller's env does any normalisation):
    env_reset() -> obs [E, O]; env_step(actions) -> (obs, rewards, dones, raw rewards).  Returns the mean raw reward of every update's rollout."""
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
