"""Inputs, fp32 emulation, bounds and fault models for tests/test_gauss_trained.py: the diagonal-Gaussian head on two tanh towers at trained-looking weights.

Every other fp32 test of this path runs at init_orthogonal weights: every bias exactly 0, |mu| <= 0.016, no tanh unit near +-1, the policy tower's hidden-layer
gradients three orders below the largest gradient entry.  A dropped bias add, a tanh that is wrong near 1, a clip gate that leaks and a hidden-layer gradient that
is 1 % off are all inside those tests' tolerances.  Here the weights are trained_theta(): scaled towers, a head of gain 1, non-zero biases everywhere, logstd in
[-3, -0.5]; the observations reach the normaliser's clip (+-10); an eighth of the minibatch sits e^+-5 deep in the ratio's clip and 2 deep in the value's.

No second reference: every expected value is oracle/torch_check.py in float64 (its forward and neglogp for the act side, loss_and_grads and clip_and_adam for the
train side, with the oracle's own ent_coef, vf_coef, max_grad_norm and Adam constants).  emulate() is NOT a reference: it is the same forward, loss and backward
written out in NumPy at a chosen dtype, in csrc/ppo_head.hpp's operand order (surrogate_row, surrogate_d_nlp, gauss_z, gauss_nlp, gauss_grad_elem, TanhGrad as
dy (1 - h h)); at float32 its tanh is fast_tanh's two forms.  At float64 it must reproduce the reference to 1e-9 (checked on the CPU); at float32 it is the stand-in
for a correct kernel, and with fault=.. for a subtly wrong one.

Bounds (bounds()): none comes from a device.  Each is the project's usual tolerance or FACTOR = 10 x the emulation's error against float64, whichever is larger
(the factor of tests/head_edges_ref.PART2_FACTOR and tests/bf16_ref.L2_FACTOR: another summation order, the hardware exp2 and rcp).  "The emulation's error" is the
largest over four correct float32 evaluations: the rows in order and reversed (another summation order of every row sum), each also with every row's neglogp moved
one float32 up or down at random (a reduction that rounds the other way).  New beside the usual rules: per parameter tensor, the relative L2 error of the gradient
is at most 10 x the emulation's and never asked below 2 x 2^-24.  The elementwise rule (rtol 2e-4, atol 2e-6 max|grad|) stays beside it.

The elementwise rule and this regime.  By itself the rule REJECTS the float32 emulation at trained weights: its worst element stands at 0.3 to 2.4 times the rule's
allowance (1.2 at 20 / 40 behind (64, 64), 1.0 to 2.4 at every (256, 256) case from 80 rows on; MEASURED's `rule` column), against 0.1 to 0.4 at the control.  The
cause is the number format, not the summation order: d loss / d mu_j = d_nlp (a_j - mu_j) / sigma_j^2, so a rounding of mu_j (1.3e-6 behind 256 units, 1e-7 at the
very best for |mu| = 2) enters that element divided by sigma_j^2, while the rule's absolute term follows the LARGEST element, which sits in a column with another
sigma; logstd spans [-3, -0.5], a factor of 150 in 1 / sigma^2.  No choice of the recipe's factors that keeps max |mu| >= 1 and min neglogp < 0 brings the
emulation under a third of the rule.  So the rule is treated as item 7 of the issue treats every other existing tolerance: an element passes inside the rule, or
inside FACTOR x the emulation's largest element error of the same tensor (bounds()["elem"]).  The same function serves the control, where the emulation stands at
0.1 to 0.4 of the rule; the files that own that regime keep applying the rule by itself.  usual_rule_ratio() reports, for the emulation and for the device, where a
gradient stands under the rule alone, and the GPU tests print it.

MEASURED: the emulation's figures at O = A = 18, trained weights (seed 3), largest over the four evaluations; test_measured_guard holds the emulation to twice them.
Beside them what an MI355X showed on the same rows (narrow_step_kernel<static> / narrow_train_kernel<static>, policy_step_kernel at 16 rows / train8_kernel +
weight_grad_assemble_kernel), for comparison only -- no bound uses a device figure:
                                     mu        value     neglogp, given actions   losses (largest of four)   gradient: largest relative L2 of a tensor   under the elementwise rule alone
    (64, 64), 33 rows     emulation  5.5e-7    9.8e-7    5.6e-6                   1.3e-6                     3.0e-5 (vf/b, one element)                   0.94
                          device     3.3e-7    6.2e-7    1.3e-5                   1.6e-6                     3.6e-5 (vf/b)                                0.38
    (256, 256), 576 rows  emulation  1.3e-6    1.6e-6    3.7e-5                   1.9e-7                     9.8e-6 (pi/b)                                1.8
                          device     4.8e-7    9.0e-7    1.1e-5                   3.5e-7                     below every bound by a factor of 10          0.71
Over all 54 GPU cases: the act and rollout figures stayed a factor of 4 or more inside their allowances (neglogp of given actions: 3.7e-5 at the most, at 36 / 40
behind (256, 256), allowance 4.3e-4); every loss a factor of 10 or more.  Per tensor, three cases came within a factor of 2 of an L2 bound, each on vf/b, the
one-element tensor, whose emulation error happens to be small: (64, 64) with 80 observations 2.3e-6 of 3.6e-6, PPO_HIP_NO_T8 at 100 rows 9.5e-7 of 1.5e-6,
PPO_HIP_NO_DW2 at 128 rows 6.6e-7 of 1.3e-6.  Under the elementwise rule ALONE the device stood at 1.16 (20 / 40 behind (64, 64)), 1.31 (PPO_HIP_NO_T8) and 1.06
(PPO_HIP_NO_DW2) at trained weights, where the emulation stands at 1.33, 1.11 and 1.88: see "The elementwise rule and this regime" above.  At the control it
stayed at or below 0.30 everywhere.
"""
import numpy as np

from oracle import oracle as o
from oracle import torch_check as tc

CR = 0.16102319955825806        # tests/test_hip_parity.CR, LR
LR = 0.000393141177482903
FACTOR = 10.0                   # tests/head_edges_ref.PART2_FACTOR, tests/bf16_ref.L2_FACTOR
L2_FLOOR = 2.0 * 2.0 ** -24     # the per-tensor bound is never tighter than two float32 roundings
BAND = 1e-3                     # tests/helpers.synth_minibatch_from's clip-edge band
FORCED_NLP, FORCED_V = 5.0, 2.0

FAULTS = ("no_hidden_bias", "no_head_bias", "tanh_clamped", "ratio_exp_clamped")        # rejected at trained weights, accepted by the control
L2_FAULTS = ("dy_bf16", "last_row_dropped")                                             # there for the per-tensor L2 rule; the control need not accept them
REPLACED_FAULTS = ("clip_pass_dropped",)                                                # see emulate()

# largest |error| of mu, of the value, of neglogp of given actions, of the four mean losses; largest per-tensor relative L2 error of the gradient (vf/b, one
# element, at 33 rows; pi/b at 576); largest gradient element error as a multiple of what the elementwise rule allows by itself (usual_rule_ratio)
MEASURED = {
    ((64, 64), 33): dict(mu=5.5e-7, v=9.8e-7, nlp=5.6e-6, loss=1.3e-6, l2=3.0e-5, rule=0.94),
    ((256, 256), 576): dict(mu=1.3e-6, v=1.6e-6, nlp=3.7e-5, loss=1.9e-7, l2=9.8e-6, rule=1.8),
}


def rne_bf16(x):
    from tests import bf16_ref as R
    return R.rne_bf16(np.asarray(x, np.float32)).astype(np.float32)


# ---- weights and observations ---------------------------------------------------------------------------------------------------------------------------------
def oracle_for(hidden, O=18, A=18):
    return o.Oracle(O, A, list(hidden))


def trained_theta(orc, seed, tower=1.5, head=100.0, vhead=3.0):
    """init_orthogonal(seed), then: first-layer weights of both towers x tower, pi/w x head (gain 1), vf/w x vhead, vf/b = 0.7, pi/b ~ U(-0.3, 0.3), every tower
    bias ~ U(-0.5, 0.5), pi/logstd ~ U(-3, -0.5); one RandomState, float32.  Returns a copy of the flat vector (orc.theta holds it too)."""
    orc.init_orthogonal(seed)
    rng = np.random.RandomState(seed + 1)
    for name, _, shape in orc.tensors:
        t = orc.tensor(name)
        if name in ("pi_fc0/w", "vf_fc0/w"):
            t *= np.float32(tower)
        elif name == "pi/w":
            t *= np.float32(head)
        elif name == "vf/w":
            t *= np.float32(vhead)
        elif name == "vf/b":
            t[:] = 0.7
        elif name == "pi/b":
            t[:] = rng.uniform(-0.3, 0.3, shape)
        elif name == "pi/logstd":
            t[:] = rng.uniform(-3.0, -0.5, shape)
        elif name.endswith("/b"):
            t[:] = rng.uniform(-0.5, 0.5, shape)
    return orc.theta.copy()


def orth_theta(orc, seed):
    """tests/test_hip_parity.pair(.., "orth")'s weights: the regime every other test runs in"""
    orc.init_orthogonal(seed)
    orc.tensor("pi/logstd")[:] = np.random.RandomState(seed + 1).uniform(-1.0, 0.2, (1, orc.A))
    return orc.theta.copy()


def trained_obs(rng, n, O):
    """U(-2, 2), a 1/16 share of the entries exactly +-10 (the normaliser's clip), row 0 all zeros"""
    obs = rng.uniform(-2.0, 2.0, (n, O))
    edge = rng.uniform(size=(n, O)) < 1.0 / 16.0
    obs[edge] = np.where(rng.uniform(size=(n, O)) < 0.5, -10.0, 10.0)[edge]
    obs[0] = 0.0
    return obs.astype(np.float32)


# ---- the float64 reference (oracle/torch_check.py) -----------------------------------------------------------------------------------------------------------------
def named64(orc, theta):
    return {name: orc.tensor(name, np.asarray(theta, np.float64)).copy() for name, _, _ in orc.tensors}


def flat64(orc, named):
    out = np.zeros(orc.P, np.float64)
    for name, _, _ in orc.tensors:
        orc.tensor(name, out)[...] = np.asarray(named[name], np.float64).reshape(orc.tensor(name, out).shape)
    return out


def ref_forward(orc, theta, obs):
    """(mu [n, A], v [n], logstd [A]) of torch_check.forward in float64"""
    import torch
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in named64(orc, theta).items()}
    mu, v, logstd = tc.forward(p, torch.tensor(np.asarray(obs, np.float64)), len(orc.hidden))
    return mu.numpy(), v.numpy(), logstd.numpy()[0]


def ref_neglogp(act, mu, logstd):
    import torch
    t = lambda x: torch.tensor(np.asarray(x, np.float64))
    return tc.neglogp(t(act), t(mu), t(np.broadcast_to(logstd, mu.shape).copy())).numpy()


# ---- minibatch -------------------------------------------------------------------------------------------------------------------------------------------------------
def synth_minibatch_from(obs, act, v, nlp, seed, cr=CR, rng=None, band=BAND):
    """tests/helpers.synth_minibatch_from with its clip-edge band as an argument (the same draws, rules and order; the pushes grow with the band)"""
    if rng is None:
        rng = np.random.RandomState(seed)
    n = obs.shape[0]
    push = max(0.01, 10.0 * band)
    old_nlp = (nlp + rng.normal(scale=0.15, size=n)).astype(np.float32)
    old_v = (v + rng.normal(scale=0.2, size=n)).astype(np.float32)
    ret = (v + rng.normal(scale=0.5, size=n)).astype(np.float32)
    ratio = np.exp(old_nlp.astype(np.float64) - nlp)
    near = np.abs(np.abs(ratio - 1.0) - cr) < band
    old_nlp[near] += np.float32(push)
    dvo = v.astype(np.float64) - old_v
    near = np.abs(np.abs(dvo) - cr) < band
    old_v[near] -= np.float32(push) * np.sign(dvo[near]).astype(np.float32)
    dvo = v.astype(np.float64) - old_v
    vclip = old_v + np.clip(dvo, -cr, cr)
    s1, s2 = (v - ret.astype(np.float64)) ** 2, (vclip - ret) ** 2
    near = (np.abs(dvo) > cr) & (np.abs(s1 - s2) < band * np.maximum(s1, 1e-6))
    ret[near] += np.float32(5.0 * push)
    adv = o.adv_normalize(ret, old_v)
    return dict(obs=obs, actions=act, advs=adv, returns=ret, old_neglogp=old_nlp, old_values=old_v)


def edge_distance(v, nlp, mb, cr=CR):
    """(distance of the nearest row to the ratio's clip edges, to the value's clip edges, smallest relative gap of the two value-loss branches on clipped rows)"""
    ratio = np.exp(mb["old_neglogp"].astype(np.float64) - nlp)
    dvo = v - mb["old_values"].astype(np.float64)
    vclip = mb["old_values"] + np.clip(dvo, -cr, cr)
    s1, s2 = (v - mb["returns"].astype(np.float64)) ** 2, (vclip - mb["returns"]) ** 2
    clipped = np.abs(dvo) > cr
    gap = (np.abs(s1 - s2) / np.maximum(s1, 1e-6))[clipped]
    return float(np.abs(np.abs(ratio - 1.0) - cr).min()), float(np.abs(np.abs(dvo) - cr).min()), float(gap.min()) if gap.size else np.inf


class Batch:
    """one case's rows: what the device and the emulation are fed, and what the float64 reference makes of it.
    kind "trained": trained_theta, trained_obs, the minibatch around the FLOAT64 outputs with the forced rows.  kind "orth": the control, pair(.., "orth") weights
    and tests/helpers.synth_minibatch (around the fp32 C oracle's outputs, obs U(-1, 1)) -- the regime of every other test."""

    def __init__(self, orc, kind, n, seed=3, mb_seed=50):
        self.orc, self.kind, self.n = orc, kind, n
        O, A = orc.O, orc.A
        if kind == "trained":
            self.theta = trained_theta(orc, seed)
            rng = np.random.RandomState(mb_seed + n)
            # (a one-row call: the second row of a two-row draw -- row 0 is the all-zero row, which every larger case has)
            self.obs = trained_obs(rng, n, O) if n > 1 else trained_obs(rng, 2, O)[1:]
            self.noise = rng.normal(size=(n, A)).astype(np.float32)
        else:
            from tests import helpers as H
            self.theta = orth_theta(orc, seed)
            rng = np.random.RandomState(mb_seed)
            self.obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
            self.noise = rng.normal(size=(n, A)).astype(np.float32)
            self.mb = H.synth_minibatch(orc, n, seed=mb_seed) if n > 1 else None
            if n > 1:
                np.testing.assert_array_equal(self.mb["obs"], self.obs)
        self.mu, self.v, self.logstd = ref_forward(orc, self.theta, self.obs)
        self.sigma = np.exp(self.logstd)
        self.a64 = self.mu + self.sigma * self.noise.astype(np.float64)               # the act model's sample, unrounded
        self.nlp_sample = ref_neglogp(self.a64, self.mu, self.logstd)
        self.ent_rows = np.full(n, (self.logstd + tc.HALF_LOG_2PIE).sum())
        self.forced = np.zeros(n, bool)
        self.band = BAND
        if kind == "trained":
            act = self.a64.astype(np.float32)
            nlp = ref_neglogp(act, self.mu, self.logstd)
            self.band = max(BAND, FACTOR * nlp_error(self, act, nlp))
            self.mb = self._trained_minibatch(act, nlp, mb_seed + 1) if n > 1 else None
        self.actions = self.mb["actions"] if n > 1 else self.a64.astype(np.float32)
        self.nlp_given = ref_neglogp(self.actions, self.mu, self.logstd)             # neglogp of the GIVEN (float32) actions: evaluate_actions, the train step

    def _trained_minibatch(self, act, nlp, seed):
        mb = synth_minibatch_from(self.obs, act, self.v, nlp, seed, band=self.band)
        n = self.n
        rows = np.argsort(np.abs(mb["advs"]), kind="stable")[:n // 8]
        sign = np.where(np.arange(rows.size) % 2 == 0, 1.0, -1.0)
        mb["old_neglogp"][rows] = (nlp[rows] + FORCED_NLP * sign).astype(np.float32)       # ratio e^+-5: deep in both clip branches
        mb["old_values"][rows] = (self.v[rows] + FORCED_V * sign).astype(np.float32)
        for _ in range(4):                                                               # (the forced rows' two value-loss branches: the band's third rule again)
            dvo = self.v - mb["old_values"].astype(np.float64)
            vclip = mb["old_values"] + np.clip(dvo, -CR, CR)
            s1, s2 = (self.v - mb["returns"].astype(np.float64)) ** 2, (vclip - mb["returns"]) ** 2
            near = (np.abs(dvo) > CR) & (np.abs(s1 - s2) < self.band * np.maximum(s1, 1e-6))
            mb["returns"][near] += np.float32(0.05)
        self.forced[rows] = True
        return mb

    def train_args(self):
        m = self.mb
        return m["obs"], m["actions"], m["advs"], m["returns"], m["old_neglogp"], m["old_values"]

    def reference_step(self):
        """dict(losses [5], grad, norm, theta, m, v) of one train step of the float64 reference from self.theta, fresh Adam slots, beta powers (beta1, beta2)"""
        orc, c = self.orc, self.orc.cfg
        named = named64(orc, self.theta)
        losses, grads = tc.loss_and_grads(named, len(orc.hidden), *self.train_args(), CR, float(c.ent_coef), float(c.vf_coef))
        return dict(losses=losses, **adam_after(orc, self.theta, flat64(orc, grads)))


class ActRows:
    """rows of an act-side comparison on GIVEN observations (the rollout tests: the device's own stored observations, teacher forcing): the fields of Batch that
    emulated_act, act_bounds and act_failures read"""

    def __init__(self, orc, theta, obs, noise):
        self.orc, self.theta, self.n = orc, np.asarray(theta, np.float32), len(obs)
        self.obs, self.noise = np.asarray(obs, np.float32), np.asarray(noise, np.float32)
        self.mu, self.v, self.logstd = ref_forward(orc, self.theta, self.obs)
        self.sigma = np.exp(self.logstd)
        self.a64 = self.mu + self.sigma * self.noise.astype(np.float64)
        self.nlp_sample = ref_neglogp(self.a64, self.mu, self.logstd)
        self.ent_rows = np.full(self.n, (self.logstd + tc.HALF_LOG_2PIE).sum())
        self.actions = self.a64.astype(np.float32)
        self.nlp_given = ref_neglogp(self.actions, self.mu, self.logstd)


def adam_after(orc, theta, grad):
    """torch_check.clip_and_adam from fresh slots on a flat gradient: dict(grad, norm, theta, m, v)"""
    c = orc.cfg
    named = named64(orc, theta)
    zeros = {k: np.zeros_like(x) for k, x in named.items()}
    g = {name: orc.tensor(name, np.asarray(grad, np.float64)) for name, _, _ in orc.tensors}
    p, m, v, _, norm = tc.clip_and_adam(named, g, zeros, zeros, (float(c.adam_beta1), float(c.adam_beta2)), LR, float(c.max_grad_norm), float(c.adam_beta1),
                                         float(c.adam_beta2), float(c.adam_eps))
    return dict(grad=np.asarray(grad, np.float64), norm=norm, theta=flat64(orc, p), m=flat64(orc, m), v=flat64(orc, v))


# ---- the same forward, loss and backward in NumPy at a chosen dtype, and its fault models -------------------------------------------------------------------------
def fast_tanh32(x):
    """ppo_kernels.hpp fast_tanh in float32: the odd polynomial x - x^3/3 + 2x^5/15 (two fused multiply-adds) below 1/16, 1 - 2 rcp(exp2(2 |x| log2 e) + 1) with
    the sign restored elsewhere"""
    f = np.float32
    x = np.asarray(x, f)
    ax, x2 = np.abs(x), x * x
    inner = (x2.astype(np.float64) * np.float64(f(0.13333333333333333)) + np.float64(f(-0.33333333333333333))).astype(f)
    p = ((x2 * x).astype(np.float64) * inner.astype(np.float64) + x.astype(np.float64)).astype(f)
    with np.errstate(over="ignore"):
        e = np.exp2(ax * f(2.8853900817779268)).astype(f)
        t = np.copysign(f(1.0) - f(2.0) * (f(1.0) / (e + f(1.0))), x).astype(f)
    return np.where(ax < f(0.0625), p, t)


def forward(orc, theta, obs, F, fault=None):
    """both towers and the heads at dtype F: dict(pre {tower: [pre-activations]}, hs {tower: [activations, input first]}, mu, v, logstd [n, A], sigma)"""
    th = np.asarray(theta, F)
    t = lambda name: orc.tensor(name, th)
    tanh = fast_tanh32 if F is np.float32 else np.tanh
    x = np.asarray(obs, F)
    hs, pre = {"pi": [x], "vf": [x]}, {"pi": [], "vf": []}
    for tw in ("pi", "vf"):
        for l in range(len(orc.hidden)):
            z = hs[tw][-1] @ t("%s_fc%d/w" % (tw, l))
            if not (fault == "no_hidden_bias" and tw == "pi" and l == 0):
                z = z + t("%s_fc%d/b" % (tw, l))
            if fault == "tanh_clamped":
                z = np.clip(z, F(-4.0), F(4.0))
            pre[tw].append(z)
            hs[tw].append(tanh(z))
    mu = hs["pi"][-1] @ t("pi/w")
    if fault != "no_head_bias":
        mu = mu + t("pi/b")
    v = (hs["vf"][-1] @ t("vf/w")).reshape(-1) + t("vf/b").reshape(-1)[0]
    logstd = mu * F(0.0) + t("pi/logstd").reshape(1, -1)                 # gauss_logstd
    return dict(pre=pre, hs=hs, mu=mu, v=v, logstd=logstd, sigma=np.exp(logstd))


def row_nlp(f, act, F):
    """gauss_z and gauss_nlp of given actions on a forward() result: (z, neglogp rows, entropy rows)"""
    A = f["mu"].shape[1]
    z = (np.asarray(act, F) - f["mu"]) / f["sigma"]
    nlp = F(0.5) * (z * z).sum(1, dtype=F) + F(tc.HALF_LOG_2PI) * F(A) + f["logstd"].sum(1, dtype=F)
    ent = (f["logstd"] + F(tc.HALF_LOG_2PIE)).sum(1, dtype=F)
    return z, nlp, ent


def nlp_error(b, act, nlp64):
    """largest |error| of the float32 emulation's neglogp of `act` against the float64 one (sets the minibatch's clip-edge band)"""
    _, nlp, _ = row_nlp(forward(b.orc, b.theta, b.obs, np.float32), act, np.float32)
    return float(np.abs(nlp.astype(np.float64) - nlp64).max())


def emulate(theta, b, dtype, fault=None, nudge=None, rev=False):
    """forward, loss and backward of Batch b at `dtype` in ppo_head.hpp's operand order.  Returns dict(pre, hs, mu, v, nlp, ent (rows), losses [5], grad [P]).
    fault --
      no_hidden_bias     the first layer's bias is not added in the policy tower
      no_head_bias       pi/b is not added
      tanh_clamped       the tanh argument is clamped to +-4 (a range-reduced tanh)
      ratio_exp_clamped  the ratio's exponent old_nlp - nlp is clamped to +-4 (a range-limited exp): only rows deep in the clip show it
      clip_pass_dropped  in surrogate_d_nlp `pass` is taken as 1.  REPLACED by ratio_exp_clamped: wherever the clipped branch is selected (sel = 0) the ratio lies
                         outside [lo, hi], so pass is 0 on exactly those rows and dropping it restores the whole unclipped gradient on EVERY clipped row, deep or
                         not.  The control has a clip fraction of 0.2 to 0.4 and rejects that at once, so the fault cannot meet its accept condition at any shape.
      dy_bf16            the policy tower's d h is rounded to bf16 before TanhGrad
      last_row_dropped   the last live row (the last one the clip lets a policy gradient through) is missing from pi_fc1/w's weight gradient only
    nudge: a RandomState; every row's neglogp is moved to the next float32 up or down at random.  rev: the rows are fed in reverse order (another summation order)."""
    F, orc = dtype, b.orc
    L, n = len(orc.hidden), b.n
    order = np.arange(n)[::-1] if rev else np.arange(n)
    obs, act, adv, ret, old_nlp, old_v = [np.ascontiguousarray(np.asarray(x)[order]).astype(F) for x in b.train_args()]
    th = np.asarray(theta, F)
    t = lambda name: orc.tensor(name, th)
    c = orc.cfg
    f = forward(orc, theta, obs, F, fault)
    mu, v, sigma, hs = f["mu"], f["v"], f["sigma"], f["hs"]
    z, nlp, ent = row_nlp(f, act, F)
    if nudge is not None:
        nlp = np.nextafter(nlp, np.where(nudge.uniform(size=n) < 0.5, -np.inf, np.inf).astype(F))
    cr = F(CR)
    g = F(1.0) / F(n)
    # surrogate_row, surrogate_d_nlp
    lo, hi = F(1.0) - cr, F(1.0) + cr
    x = old_nlp - nlp
    if fault == "ratio_exp_clamped":
        x = np.clip(x, F(-4.0), F(4.0))
    ratio = np.exp(x)
    rmin = np.minimum(ratio, hi)
    rclip = np.maximum(rmin, lo)
    m1, m2 = -adv * ratio, -adv * rclip
    sel = (m1 >= m2).astype(F)
    pas = (rmin >= lo).astype(F) * (ratio <= hi).astype(F)
    if fault == "clip_pass_dropped":
        pas = np.ones_like(pas)
    d_ratio = (-adv) * g * sel
    d_ratio = d_ratio + (-adv) * g * (F(1.0) - sel) * pas
    d_nlp = -(d_ratio * ratio)
    # gauss_grad_elem
    dl = d_nlp[:, None] * (F(1.0) - z * z) - F(c.ent_coef) * g
    dmu = d_nlp[:, None] * (-(z / sigma)) + dl * F(0.0)
    # value loss: 0.5 mean max((v - R)^2, (vclip - R)^2), TF's tie rules (oracle/numpy_port.py)
    dvo = v - old_v
    vmin = np.minimum(dvo, cr)
    vclip = old_v + np.maximum(vmin, -cr)
    e1, e2 = v - ret, vclip - ret
    s1, s2 = e1 * e1, e2 * e2
    gv = F(c.vf_coef) * F(0.5) * g
    selv = (s1 >= s2).astype(F)
    passv = (vmin >= -cr).astype(F) * (dvo <= cr).astype(F)
    d_v = gv * selv * (F(2.0) * e1) + gv * (F(1.0) - selv) * (F(2.0) * e2) * passv
    dk = nlp - old_nlp
    losses = np.array([np.maximum(m1, m2).mean(dtype=F), F(0.5) * np.maximum(s1, s2).mean(dtype=F), ent.mean(dtype=F), F(0.5) * (dk * dk).mean(dtype=F),
                       (np.abs(ratio - F(1.0)) > cr).mean()], np.float64)
    grad = np.zeros(orc.P, F)
    put = lambda name, val: orc.tensor(name, grad).__setitem__(Ellipsis, np.asarray(val, F).reshape(orc.tensor(name, grad).shape))
    put("pi/logstd", dl.sum(0, dtype=F))
    put("pi/w", hs["pi"][-1].T @ dmu)
    put("pi/b", dmu.sum(0, dtype=F))
    put("vf/w", hs["vf"][-1].T @ d_v[:, None])
    put("vf/b", d_v.sum(dtype=F))
    for tw, dh in (("pi", dmu @ t("pi/w").T), ("vf", d_v[:, None] * t("vf/w").reshape(1, -1))):
        for l in range(L - 1, -1, -1):
            y = hs[tw][l + 1]
            if fault == "dy_bf16" and tw == "pi":
                dh = rne_bf16(dh).astype(F)
            dz = dh * (F(1.0) - y * y)                                      # TanhGrad
            if fault == "last_row_dropped" and tw == "pi" and l == 1:
                live = order != np.nonzero(np.asarray(d_nlp)[np.argsort(order)])[0][-1]      # (the last row that has a policy gradient at all: a clipped row adds none)
                put("pi_fc1/w", hs[tw][l][live].T @ dz[live])
            else:
                put("%s_fc%d/w" % (tw, l), hs[tw][l].T @ dz)
            put("%s_fc%d/b" % (tw, l), dz.sum(0, dtype=F))
            if l:
                dh = dz @ t("%s_fc%d/w" % (tw, l)).T
    back = np.argsort(order)
    rows = lambda a: np.asarray(a)[back]
    return dict(pre={k: [rows(a) for a in x] for k, x in f["pre"].items()}, hs={k: [rows(a) for a in x] for k, x in hs.items()}, mu=rows(mu), v=rows(v),
                nlp=rows(nlp), ent=rows(ent), losses=losses, grad=grad.astype(np.float64))


def emulated_act(b, fault=None):
    """what an fp32 kernel returns from one call each of step (explicit noise), value, act_deterministic and evaluate_actions"""
    F = np.float32
    f = forward(b.orc, b.theta, b.obs, F, fault)
    a = f["mu"] + f["sigma"] * b.noise                                       # gauss_sample
    _, nlp_step, _ = row_nlp(f, a, F)
    _, nlp_eval, ent = row_nlp(f, b.actions, F)
    return dict(action=a, value_step=f["v"], nlp_step=nlp_step, value=f["v"], mu=f["mu"], value_eval=f["v"], nlp_eval=nlp_eval, ent=ent)


def emulated_train(b, fault=None, dtype=np.float32, nudge=None, rev=False):
    """what an fp32 kernel leaves after one train step: dict(losses, grad, norm, theta, m, v)"""
    e = emulate(b.theta, b, dtype, fault, nudge, rev)
    return dict(losses=e["losses"], **adam_after(b.orc, b.theta, e["grad"]))


# ---- conditions on the inputs ------------------------------------------------------------------------------------------------------------------------------------
def input_stats(b):
    """from the float64 forward alone: dict(sat {tower: share of first-layer units with |h| > 0.99}, poly: smallest share over the layers of both towers of
    pre-activations with |x| < 1/16, mu_max, nlp_min, zero_biases: names of bias tensors that are all zero)"""
    f = forward(b.orc, b.theta, b.obs, np.float64)
    _, nlp, _ = row_nlp(f, b.actions, np.float64)
    sat = {tw: float((np.abs(f["hs"][tw][1]) > 0.99).mean()) for tw in ("pi", "vf")}
    poly = min(float((np.abs(x) < 0.0625).mean()) for tw in ("pi", "vf") for x in f["pre"][tw])
    zero = [name for name, _, _ in b.orc.tensors if name.endswith("/b") and not np.any(b.orc.tensor(name, b.theta))]
    return dict(sat=sat, poly=poly, mu_max=float(np.abs(f["mu"]).max()), nlp_min=float(nlp.min()), zero_biases=zero)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------------------------------
def tensor_l2(orc, got, want):
    """{tensor: relative L2 error of got against want} over the flat gradient vectors"""
    out = {}
    for name, _, _ in orc.tensors:
        w = orc.tensor(name, want)
        out[name] = float(np.linalg.norm(orc.tensor(name, got) - w) / np.linalg.norm(w)) if np.any(w) else float(np.abs(orc.tensor(name, got)).max())
    return out


def act_bounds(b):
    """dict(mu, v, nlp: absolute allowances beside the usual tolerances; measured: the emulation's errors).  Forward only: any row count."""
    e = emulated_act(b)
    meas = dict(mu=float(np.abs(e["mu"] - b.mu).max()), v=float(np.abs(e["value"] - b.v).max()),
                nlp=float(max(np.abs(e["nlp_eval"] - b.nlp_given).max(), np.abs(e["nlp_step"] - b.nlp_sample).max())))
    return dict(mu=FACTOR * meas["mu"], v=FACTOR * meas["v"], nlp=FACTOR * meas["nlp"], measured=meas)


def bounds(b, want=None):
    """act_bounds plus the train side's: loss [4] absolute allowances, l2 {tensor: bound}, norm (relative), theta / m / adam_v (absolute), each FACTOR x the largest
    error over the four correct float32 evaluations (rows in order / reversed, neglogp as computed / nudged) against the float64 reference"""
    out = act_bounds(b)
    want = want or b.reference_step()
    orc = b.orc
    worst = dict(loss=np.zeros(4), l2={name: 0.0 for name, _, _ in orc.tensors}, elem={name: 0.0 for name, _, _ in orc.tensors}, rule=0.0, norm=0.0, theta=0.0, m=0.0, adam_v=0.0, nlp=out["measured"]["nlp"])
    for i, (rev, nudged) in enumerate(((False, False), (True, False), (False, True), (True, True))):
        e = emulate(b.theta, b, np.float32, None, np.random.RandomState(900 + i) if nudged else None, rev)
        got = adam_after(orc, b.theta, e["grad"])
        worst["loss"] = np.maximum(worst["loss"], np.abs(e["losses"][:4] - want["losses"][:4]))
        for name, x in tensor_l2(orc, e["grad"], want["grad"]).items():
            worst["l2"][name] = max(worst["l2"][name], x)
            worst["elem"][name] = max(worst["elem"][name], float(np.abs(orc.tensor(name, e["grad"]) - orc.tensor(name, want["grad"])).max()))
        worst["rule"] = max(worst["rule"], usual_rule_ratio(e["grad"], want["grad"]))
        worst["norm"] = max(worst["norm"], abs(got["norm"] - want["norm"]) / want["norm"])
        worst["theta"] = max(worst["theta"], float(np.abs(got["theta"] - want["theta"]).max()))
        worst["m"] = max(worst["m"], float(np.abs(got["m"] - want["m"]).max()))
        worst["adam_v"] = max(worst["adam_v"], float(np.abs(got["v"] - want["v"]).max()))
        if not nudged:
            worst["nlp"] = max(worst["nlp"], float(np.abs(e["nlp"] - b.nlp_given).max()))
    out["measured"].update(worst)
    out.update(nlp=FACTOR * worst["nlp"], loss=FACTOR * worst["loss"], l2={k: max(FACTOR * x, L2_FLOOR) for k, x in worst["l2"].items()},
               elem={k: FACTOR * x for k, x in worst["elem"].items()}, norm=FACTOR * worst["norm"],
               theta=FACTOR * worst["theta"], m=FACTOR * worst["m"], adam_v=FACTOR * worst["adam_v"])
    return out


# ---- the assertions: the GPU tests and the CPU tests of their teeth call the same functions ---------------------------------------------------------------------------
def _within(got, want, floor, extra):
    return np.abs(np.asarray(got, np.float64) - want) <= np.maximum(floor, extra)


def act_failures(b, got, bnd, keys=None):
    """names of the act-side assertions that `got` (emulated_act's keys, or some of them) fails: finite, mu, value, action, neglogp, entropy"""
    A = b.orc.A
    fails = []
    usual = lambda w: 1e-5 + 1e-4 * np.abs(w)
    rules = (("mu", "mu", b.mu, usual(b.mu), bnd["mu"]), ("action", "action", b.a64, usual(b.a64), bnd["mu"]),
             ("value_step", "value", b.v, usual(b.v), bnd["v"]), ("value", "value", b.v, usual(b.v), bnd["v"]), ("value_eval", "value", b.v, usual(b.v), bnd["v"]),
             ("nlp_step", "neglogp", b.nlp_sample, 1e-5 * A + 1e-4 * np.abs(b.nlp_sample), bnd["nlp"]),
             ("nlp_eval", "neglogp", b.nlp_given, 1e-5 * A + 1e-4 * np.abs(b.nlp_given), bnd["nlp"]),
             ("ent", "entropy", b.ent_rows, usual(b.ent_rows), 0.0))
    for key, name, want, floor, extra in rules:
        if key not in got or (keys and key not in keys):
            continue
        x = np.asarray(got[key], np.float64)
        if not np.isfinite(x).all():
            fails.append("finite: %s" % key)
        elif not _within(x, want, floor, extra).all():
            err = np.abs(x - want)
            fails.append("%s: %s off by %.3g at %s (allowed %.3g)" % (name, key, err.max(), np.unravel_index(err.argmax(), err.shape), float(np.max(np.maximum(floor, extra)))))
    return fails


def train_failures(b, got, want, bnd):
    """names of the train-side assertions that `got` fails: finite, pg_loss, vf_loss, entropy, approxkl, clipfrac, grad elementwise, grad L2 <tensor>, norm, theta,
    adam m, adam v.  got / want: dict(losses, grad, norm, theta, m, v)."""
    orc, n = b.orc, b.n
    fails = []
    for k in ("losses", "grad", "norm", "theta", "m", "v"):
        if not np.isfinite(got[k]).all():
            fails.append("finite: %s" % k)
    if fails:
        return fails
    gl, wl = np.asarray(got["losses"], np.float64), want["losses"]
    for i, name in enumerate(("pg_loss", "vf_loss", "entropy", "approxkl")):
        if not _within(gl[i], wl[i], 1e-6 + 1e-4 * abs(wl[i]), bnd["loss"][i]):
            fails.append("%s: %.9g against %.12g (allowed %.3g)" % (name, gl[i], wl[i], max(1e-6 + 1e-4 * abs(wl[i]), bnd["loss"][i])))
    if abs(gl[4] - wl[4]) > 1.0 / n + 1e-6:
        fails.append("clipfrac: %.6g against %.6g" % (gl[4], wl[4]))
    grad, ref = np.asarray(got["grad"], np.float64), want["grad"]
    gs = float(np.abs(ref).max())
    extra = np.zeros(orc.P)
    for name, _, _ in orc.tensors:
        orc.tensor(name, extra)[...] = bnd["elem"][name]
    bad = ~_within(grad, ref, 2e-6 * gs + 2e-4 * np.abs(ref), extra)
    if bad.any():
        fails.append("grad elementwise: %d elements, the first at %d" % (bad.sum(), int(np.argmax(bad))))
    for name, x in tensor_l2(orc, grad, ref).items():
        if x > bnd["l2"][name]:
            fails.append("grad L2 %s: %.3g (bound %.3g)" % (name, x, bnd["l2"][name]))
    if abs(got["norm"] - want["norm"]) > max(1e-4, bnd["norm"]) * want["norm"]:
        fails.append("norm: %.9g against %.12g" % (got["norm"], want["norm"]))
    for key, name, rtol, atol in (("theta", "theta", 1e-4, 2e-6), ("m", "adam m", 2e-4, 1e-7 * max(1.0, gs)), ("v", "adam v", 4e-4, 1e-10)):
        bad = ~_within(got[key], want[key], atol + rtol * np.abs(want[key]), bnd["adam_v" if key == "v" else key])
        if bad.any():
            fails.append("%s: %d elements, the first at %d" % (name, bad.sum(), int(np.argmax(bad))))
    return fails


def usual_rule_ratio(grad, ref):
    """largest |error| of a gradient element as a multiple of what the elementwise rule allows WITHOUT the emulation's allowance (above 1: the rule alone rejects)"""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(grad, np.float64) - ref) / (2e-6 * np.abs(ref).max() + 2e-4 * np.abs(ref))).max())


def l2_report(b, got, want, bnd):
    """(tensor, relative L2 error, bound) of the tensor nearest its bound"""
    l2 = tensor_l2(b.orc, np.asarray(got["grad"], np.float64), want["grad"])
    name = max(l2, key=lambda k: l2[k] / bnd["l2"][k])
    return name, l2[name], bnd["l2"][name]
