"""Multi-binary policies (MultiBinary action spaces, stable-baselines' BernoulliProbabilityDistribution) on the fp32 path:
ppo_create_ex(..., PPO_ACT_MULTI_BINARY) / PPOHip(action_dist="multi_binary") against tests/bernoulli_ref.py (float64 NumPy forward, torch float64 autograd of the
smooth identity softplus(l) - l z for the loss and its gradient).

CPU tests: the define and the keyword exist, there is no CPU fallback, the reference's gradient is right, the stated float32 form stays within the act
tolerances at trained-policy logits, three fault models are each rejected by a named assertion.
GPU tests: act / trained logits / on-device draws / train / rollouts / update / kernel selection / errors / tensor round trip / checkpoint / data parallel / learning.

Tolerances are those of tests/test_discrete_policy.py (which takes them from tests/test_hip_parity.py): act 1e-4 / 1e-5; losses 1e-4 / 1e-6; clipfrac within a
row; gradient 2e-4 with 2e-6 of its largest element; norm 1e-4; theta 1e-4 / 2e-6; Adam m 2e-4; rollout fields 2e-4 / 2e-5.  None is derived here."""
import ctypes
import os

import numpy as np
import pytest

from tests.bernoulli_ref import BernRef, bern_stats, emulate_f32
from tests.head_edges_ref import FORCED_ADV, synth_from
from tests.test_discrete_policy import CR, GAMMA, LAM, LR, close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, MOVE = 1e-4, 2e-4      # a uniform within NEAR of its p is moved to p +- MOVE: the device's logit error of 1e-5 moves p by 3e-6 at most (|dp/dl| <= 1/4)
DET_TIE = 1e-5               # a deterministic bit may go either way where |logit| is below the device's logit error
TINY = np.float32(2.0 ** -126)            # the smallest positive normal float32
LAST = np.float32(1.0 - 2.0 ** -24)       # the largest float32 below 1


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_define_and_action_dist_entry_exist():
    src = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    assert "#define PPO_ACT_MULTI_BINARY 3" in src
    assert "#define PPO_ACT_GAUSSIAN    0" in src and "#define PPO_ACT_CATEGORICAL 1" in src and "#define PPO_ACT_MULTI_CATEGORICAL 2" in src
    assert "#define PPO_ABI_VERSION 3" in src
    from ppo_cpp_amd import capi
    assert capi.ACTION_DISTS["multi_binary"] == 3
    assert "bernoulli" not in capi.ACTION_DISTS


def test_multi_binary_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import ppo_cpp_amd
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="no CPU fallback"):
        ppo_cpp_amd.PPOHip(18, 6, [4, 5], action_dist="multi_binary")


def test_source_names_the_head_in_every_layer():
    """the counters, the pickers and the host layer know the head (fails on a tree without it; runs nothing)"""
    hip = open(os.path.join(ROOT, "ppo_cpp_amd", "csrc", "ppo_hip.hip")).read()
    assert '"policy_step_kernel<mbin>"' in hip and '"train_fwd_bwd_kernel<mbin>"' in hip
    assert "static_assert(KV_COUNT <= 64" in hip
    head = open(os.path.join(ROOT, "ppo_cpp_amd", "csrc", "ppo_head.hpp")).read()
    for piece in ("bern_parts", "bern_nlp_elem", "bern_entropy_elem", "bern_grad_elem"):
        assert piece in head, piece
    mixin = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "env", "multi_binary.hpp")).read()
    assert "struct IMultiBinary" in mixin and "binary_actions_of(Env*" in mixin
    host = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "ppo_host.cpp")).read()
    assert "int ppo_host_learn_binary(" in host and "int ppo_host_binary_checkpoint(" in host


def test_bernoulli_is_still_no_action_dist():
    import ppo_cpp_amd
    with pytest.raises(ValueError, match="action_dist"):
        ppo_cpp_amd.PPOHip(18, 6, [4, 5], action_dist="bernoulli")


def small_case(ent_coef=0.05, n=12, seed=3):
    ref = BernRef(5, 4, [6, 3], ent_coef=ent_coef)
    ref.init_random(seed)
    rng = np.random.RandomState(0)
    obs = rng.uniform(-1, 1, (n, 5))
    x, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, 4)))
    old_nlp = nlp + rng.normal(scale=0.05, size=n)
    old_v = v + rng.normal(scale=0.05, size=n)
    ret = v + rng.normal(scale=0.5, size=n)
    adv = rng.normal(size=n)
    return ref, (obs, x, adv, ret, old_nlp, old_v, 0.3)


def test_reference_gradient_matches_central_differences():
    """The autograd arbiter itself: d loss / d theta against central finite differences of the float64 NumPy loss (another statement of the same loss)."""
    ref, args = small_case()
    l5, grad = ref.loss_grad(*args)
    np.testing.assert_allclose(l5[0] - ref.ent * l5[2] + ref.vfc * l5[1], ref.loss_value(ref.theta, *args), rtol=1e-12)
    h = 1e-6
    fd = np.empty(ref.P)
    for i in range(ref.P):
        tp, tm = ref.theta.copy(), ref.theta.copy()
        tp[i] += h; tm[i] -= h
        fd[i] = (ref.loss_value(tp, *args) - ref.loss_value(tm, *args)) / (2 * h)
    np.testing.assert_allclose(grad, fd, rtol=1e-5, atol=1e-8)


def spread_logits(spread, n=4096, A=18, seed=0):
    rng = np.random.RandomState(seed)
    return (rng.uniform(-spread, spread, (n, A))).astype(np.float32), rng.uniform(size=(n, A)).astype(np.float32)


def robust(u, logits):
    """elements whose bit does not depend on an error of 1e-4 in p"""
    p = bern_stats(logits)[0]
    return np.abs(u.astype(np.float64) - p) >= NEAR


@pytest.mark.parametrize("spread", [1.5, 40.0, 120.0])
def test_float32_form_stays_within_the_act_tolerances(spread):
    """the form stated in include/ppo_hip.h, in float32 NumPy, against float64 at 4096 x 18 logits: neglogp and entropy within the act tolerance 1e-4 / 1e-5, every
    sampled bit the float64 choice outside |u - p| < 1e-4, nothing overflows or gives a NaN"""
    l, u = spread_logits(spread)
    p64, nlp1, nlp0, ent = bern_stats(l)
    p, x, nlp, H, pq = emulate_f32(l, u=u)
    assert np.isfinite(p).all() and np.isfinite(nlp).all() and np.isfinite(H).all() and np.isfinite(pq).all()
    ok = robust(u, l)
    np.testing.assert_array_equal(x[ok], (u.astype(np.float64) < p64)[ok].astype(np.float32))
    want = np.where(x > 0, nlp1, nlp0).sum(axis=1)
    print("spread %g: neglogp abs err %.3g, entropy abs err %.3g" % (spread, np.abs(nlp - want).max(), np.abs(H - ent.sum(axis=1)).max()))
    close(nlp, want, msg="neglogp")
    close(H, ent.sum(axis=1), msg="entropy")
    close(pq, p64 * (1.0 - p64), msg="p (1 - p)")


# the three assertions the fault models are held against: each takes the emulation's outputs (or a faulted variant) and the float64 reference
def assert_bits_follow_p(x, u, l):
    ok = robust(u, l)
    np.testing.assert_array_equal(x[ok], (u.astype(np.float64) < bern_stats(l)[0])[ok].astype(np.float32), err_msg="sampled bits")


def assert_entropy(H, l):
    close(H, bern_stats(l)[3].sum(axis=1), msg="entropy")


def assert_dlogits(dl, ref_dl):
    close(dl, ref_dl, rtol=2e-4, atol=2e-6 * np.abs(ref_dl).max(), msg="d logits")


def dlogits_f32(l, x, d_nlp, ent_coef, g, entropy_term=True):
    f = np.float32
    p, _, _, _, pq = emulate_f32(l, x=x)
    out = f(d_nlp)[:, None] * (p - x)
    if entropy_term:
        out = out + f(ent_coef) * f(g) * (l * pq)
    return out.astype(f)


def dlogits_f64(l, x, d_nlp, ent_coef, g):
    """torch float64 autograd of sum_rows d_nlp_row neglogp_row - ent_coef g sum_rows entropy_row with the smooth identity"""
    import torch
    t = torch.tensor(np.asarray(l, np.float64), requires_grad=True)
    sp = torch.nn.functional.softplus
    nlp = (sp(t) - t * torch.tensor(np.asarray(x, np.float64))).sum(1)
    ent = (sp(t) - t * torch.sigmoid(t)).sum(1)
    ((torch.tensor(np.asarray(d_nlp, np.float64)) * nlp).sum() - ent_coef * g * ent.sum()).backward()
    return t.grad.numpy()


def test_three_fault_models_are_each_rejected_and_the_true_form_passes():
    l, u = spread_logits(1.5, n=256)
    f = np.float32
    p, x, nlp, H, pq = emulate_f32(l, u=u)
    n, ent_coef = len(l), 0.01
    g = 1.0 / n
    d_nlp = (np.random.RandomState(4).normal(size=n) * g).astype(f)
    ref_dl = dlogits_f64(l, x, d_nlp, ent_coef, g)
    # the true form passes all three
    assert_bits_follow_p(x, u, l)
    assert_entropy(H, l)
    assert_dlogits(dlogits_f32(l, x, d_nlp, ent_coef, g), ref_dl)
    # x = u < 1 - p
    with pytest.raises(AssertionError, match="sampled bits"):
        assert_bits_follow_p((u < f(1) - p).astype(f), u, l)
    # entropy's |l| q term dropped
    with pytest.raises(AssertionError, match="entropy"):
        assert_entropy(np.log1p(np.exp(-np.abs(l), dtype=f), dtype=f).sum(axis=1, dtype=f), l)
    # d l = d_nlp (p - x) without the entropy term at ent_coef = 0.01
    with pytest.raises(AssertionError, match="d logits"):
        assert_dlogits(dlogits_f32(l, x, d_nlp, ent_coef, g, entropy_term=False), ref_dl)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def make(O, A, hidden, seed=0, pi_gain=1.0, flags=None, **overrides):
    import ppo_cpp_amd
    g = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="multi_binary", **dict(flags or {}), **overrides)
    c = g.cfg
    ref = BernRef(O, A, hidden, ent_coef=c.ent_coef, vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm, beta1=c.adam_beta1,
                  beta2=c.adam_beta2, eps=c.adam_eps)
    ref.init_random(seed, pi_gain)
    g.set_flat(ref.theta.astype(np.float32))
    return ref, g


def clear_uniforms(ref, obs, u):
    """every uniform within NEAR of the reference's p moves to p +- MOVE, on the side it was on: no element is skipped afterwards"""
    p = bern_stats(ref.forward(obs)[0])[0]
    u = np.array(u, np.float32)
    near = np.abs(u.astype(np.float64) - p) < NEAR
    u[near] = np.where(u[near].astype(np.float64) < p[near], p[near] - MOVE, p[near] + MOVE).astype(np.float32)
    assert (np.abs(u.astype(np.float64) - p) >= NEAR).all()
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("O,A,hidden", [(7, 1, (4, 5)), (18, 6, (64, 64)), (18, 18, (256, 256)), (50, 40, (256, 256)), (256, 64, (1024, 1024))])
@pytest.mark.parametrize("n", [1, 17, 300])
def test_step_matches_reference(O, A, hidden, n):
    ref, g = make(O, A, hidden, seed=n, pi_gain=3.0)
    assert g.lib.ppo_action_dist(g.h) == 3 and g.action_width == A and g.nvec == []
    names = [t[0] for t in g.tensors]
    assert "pi/logstd" not in names and len(names) == 4 * len(hidden) + 4
    assert dict(g.tensors)["pi/w"] == (hidden[-1], A) and dict(g.tensors)["pi/b"] == (A,)
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    u = clear_uniforms(ref, obs, rng.uniform(size=(n, A)))
    x, v, nlp = g.step(obs, u)
    assert x.shape == (n, A) and v.shape == (n,) and nlp.shape == (n,)
    rx, rv, rnlp, _ = ref.step(obs, u)
    np.testing.assert_array_equal(x, rx.astype(np.float32), err_msg="sampled bits")
    close(nlp, rnlp, msg="neglogp")
    close(v, rv, msg="value")
    close(g.value(obs), rv, msg="ppo_value")
    logits = ref.forward(obs)[0]
    det = g.act_deterministic(obs)
    assert det.shape == (n, A)
    sure = np.abs(logits) >= DET_TIE
    np.testing.assert_array_equal(det[sure], (logits > 0)[sure].astype(np.float32), err_msg="deterministic bits")
    assert set(np.unique(det)) <= {0.0, 1.0}
    kc = g.kernel_counts()
    assert kc["policy_step_kernel<mbin>"] > 0 and kc["policy_step_kernel"] == 0, kc
    g.close()


# pi/w = 0 and pi/b = a row of this table: the logits are the bias bit for bit
def logit_table(A=18):
    alt = np.where(np.arange(A) % 2 == 0, 1.0, -1.0)
    return {"pm40": 40.0 * alt, "pm120": 120.0 * alt, "all-200": np.full(A, -200.0), "all+3072": np.full(A, 3072.0),
            "zeros": np.where(np.arange(A) % 2 == 0, 0.0, -0.0), "control": np.linspace(-1.5, 1.5, A)}


def trained_case(ref, name, bias, n, seed=5):
    """theta with pi/w = 0 and pi/b = bias; observations; uniforms (cleared of near-ties, then the two edge values planted); the reference's bits with the unlikely
    value forced, as tests/head_edges_ref.train_actions places it: on the n // 5 rows with the smallest |adv| that have |adv| <= FORCED_ADV (the smallest in any case),
    bit row % A, so that a forced bit weighs at most 0.1 / n in the gradient"""
    A, O = ref.A, ref.O
    ref.init_random(seed)
    ref.t("pi/w")[:] = 0.0
    ref.t("pi/b")[:] = bias
    ref.theta[:] = ref.theta.astype(np.float32)
    rng = np.random.RandomState(seed + 1)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    logits, v = ref.forward(obs)
    np.testing.assert_array_equal(logits, np.broadcast_to(np.asarray(bias, np.float32).astype(np.float64), (n, A)))
    u = clear_uniforms(ref, obs, rng.uniform(size=(n, A)))
    u[0, :] = TINY
    u[1, :] = LAST
    p = bern_stats(logits)[0]
    # the planted values are robust too: the logits are exact, so the device's p differs from float64's by the rounding of the stated float32 form and by its
    # exp's error only -- the bit is the float64 one for the form evaluated with e (1 +- 1e-5)
    f = np.float32
    for s in (1 - 1e-5, 1 + 1e-5):
        e = (np.exp(-np.abs(logits[:2])) * s).astype(f)
        p32 = np.where(logits[:2] >= 0, f(1) / (f(1) + e), e / (f(1) + e)).astype(f)
        np.testing.assert_array_equal(u[:2] < p32, u[:2].astype(np.float64) < p[:2])
    x, _, _, _ = ref.step(obs, u)
    adv, ret, _, old_v = synth_from(v, np.zeros(n), seed + 2)            # (the advantages do not depend on the actions)
    order = np.argsort(np.abs(adv), kind="stable")[:n // 5]
    forced = np.zeros(n, bool)
    forced[order] = True
    forced &= np.abs(adv) <= FORCED_ADV
    forced[order[:1]] = True
    xt = x.copy()
    for i in np.nonzero(forced)[0]:
        xt[i, i % A] = 0.0 if logits[i, i % A] > 0 else 1.0               # the less likely value (a logit of +-0: 1, neglogp log 2 either way)
    nlp_t, ent = ref.neglogp_entropy(obs, xt)
    adv2, ret2, old_nlp, old_v2 = synth_from(v, nlp_t, seed + 2)
    np.testing.assert_array_equal(adv, adv2)
    return dict(obs=obs, u=u, x=x, xt=xt, logits=logits, v=v, ent=ent, forced=forced, adv=adv, ret=ret2, old_nlp=old_nlp, old_v=old_v2, nlp_t=nlp_t)


@pytest.mark.gpu
def test_trained_logits():
    from tests.test_head_edges import assert_padding_gradient_is_zero, bias_word, reset
    O, A, hidden, n = 18, 18, (64, 64), 32
    ref, g = make(O, A, hidden, ent_coef=0.01)
    pw0 = g.beta_powers()
    at = bias_word(g, ref)
    for name, bias in logit_table(A).items():
        c = trained_case(ref, name, bias, n)
        theta0 = ref.theta.copy()
        reset(g, theta0, pw0)
        ref.m[:] = 0; ref.v[:] = 0; ref.pow = [ref.b1, ref.b2]
        x, v, nlp = g.step(c["obs"], c["u"])
        np.testing.assert_array_equal(x, c["x"].astype(np.float32), err_msg=name + " sampled bits")
        p = bern_stats(c["logits"])[0]
        assert (x[p == 1.0] == 1.0).all() and (x[p == 0.0] == 0.0).all(), name
        rnlp, _ = ref.neglogp_entropy(c["obs"], c["x"])
        close(nlp, rnlp, msg=name + " neglogp")
        close(v, c["v"], msg=name + " value")
        det = g.act_deterministic(c["obs"])
        np.testing.assert_array_equal(det, (c["logits"] > 0).astype(np.float32), err_msg=name + " deterministic bits")
        if name == "zeros":
            assert not det.any(), "a logit of +-0 acts 0 deterministically"
        if name == "all+3072":
            assert (x == 1.0).all()
        if name == "all-200":
            assert (x == 0.0).all()
        batch = (c["obs"], c["xt"].astype(np.float32), c["adv"], c["ret"], c["old_nlp"], c["old_v"])
        losses = g.train_step(LR, CR, *batch)
        grad, norm = g.last_grad()
        ref_losses, ref_grad = ref.train_step(LR, CR, *batch)
        print("%s: forced rows %d, losses %s" % (name, c["forced"].sum(), losses))
        close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg=name + " losses")
        close(losses[2], c["ent"].mean(), rtol=1e-4, atol=1e-6, msg=name + " entropy")
        assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, (name, "clipfrac", losses[4], ref_losses[4])
        gs = np.abs(ref_grad).max()
        close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg=name + " grad")
        close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg=name + " norm")
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg=name + " theta")
        close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg=name + " adam m")
        for t in ("pi_fc0/w", "pi_fc0/b", "pi_fc1/w", "pi_fc1/b"):          # pi/w = 0: nothing flows below the head, exactly
            o, shape = ref.offs[t]
            assert not grad[o:o + int(np.prod(shape))].any(), (name, t)
        assert_padding_gradient_is_zero(g, at, A, name)
    g.close()


@pytest.mark.gpu
def test_on_device_draws_are_the_counter_models():
    from tests import counter_draws_ref as M
    O, A, E, T, key = 18, 18, 64, 16, 1234
    ref, g = make(O, A, (64, 64), seed=2)
    ref.t("pi/w")[:] = 0.0
    ref.t("pi/b")[:] = np.linspace(-4, 4, A)
    ref.theta[:] = ref.theta.astype(np.float32)
    g.set_flat(ref.theta.astype(np.float32))
    p = bern_stats(ref.t("pi/b").reshape(1, A))[0]
    model = np.stack([M.counter_uniforms(key, np.arange(E), t, A) for t in range(T)])          # [T, E, A]
    assert (np.abs(model - p) >= 2.0 ** -16).all(), "a model uniform lies within 2^-16 of its p"    # nothing is skipped below
    g.rollout_alloc(E, T)                                     # (no norm_init: normalisation off)
    g.collect_synthetic(key, GAMMA, LAM, None, env0=0, step0=0)
    bits = g.rollout_get("actions")
    assert bits.shape == (T, E, A)
    np.testing.assert_array_equal(bits, (model < p).astype(np.float32))
    freq = bits.reshape(T * E, A).mean(axis=0)
    bound = 5 * np.sqrt(p[0] * (1 - p[0]) / (T * E)) + 1.0 / (T * E)
    assert (np.abs(freq - p[0]) <= bound).all(), (freq, p[0])
    nlp1, nlp0 = bern_stats(ref.t("pi/b").reshape(1, A))[1:3]
    close(g.rollout_get("neglogp"), np.where(bits > 0, nlp1, nlp0).sum(axis=2), rtol=2e-4, atol=2e-5, msg="neglogp of the drawn bits")
    obs = np.random.RandomState(2).uniform(-1, 1, (64, O)).astype(np.float32)
    g.seed(11)
    a1, _, _ = g.step(obs)
    g.seed(11)
    a2, _, _ = g.step(obs)
    np.testing.assert_array_equal(a1, a2)
    g.seed(12)
    a3, _, _ = g.step(obs)
    assert not np.array_equal(a3, a1)
    g.close()


def synth_batch(ref, n, seed, cr=CR):
    """tests/test_discrete_policy.synth_batch's recipe with this head's actions: rows 1e-3 clear of the loss's discontinuities (tests/head_edges_ref.synth_from is
    that recipe around given reference outputs)"""
    rng = np.random.RandomState(seed)
    obs = rng.uniform(-1, 1, (n, ref.O)).astype(np.float32)
    x, v, nlp, _ = ref.step(obs, rng.uniform(size=(n, ref.A)))
    adv, ret, old_nlp, old_v = synth_from(v, nlp, seed + 1000, cr)
    return obs, x.astype(np.float32), adv, ret, old_nlp, old_v


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,n", [((64, 64), 200), ((256, 256), 72)])
def test_three_train_steps_match_reference(hidden, n):
    ref, g = make(18, 18, hidden, seed=9, ent_coef=0.01)
    for it in range(3):
        batch = synth_batch(ref, n, 100 + it)
        losses = g.train_step(LR, CR, *batch)
        grad, norm = g.last_grad()
        ref_losses, ref_grad = ref.train_step(LR, CR, *batch)
        close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="losses it=%d" % it)
        assert abs(losses[4] - ref_losses[4]) <= 1.0 / n + 1e-6, ("clipfrac", losses[4], ref_losses[4])
        gs = np.abs(ref_grad).max()
        close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg="grad it=%d" % it)
        close(norm, np.sqrt(np.dot(ref_grad, ref_grad)), rtol=1e-4, msg="norm it=%d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=2e-6, msg="theta it=%d" % it)
        close(g.get_flat(1), ref.m, rtol=2e-4, atol=1e-7 * max(1.0, gs), msg="adam m it=%d" % it)
    kc = g.kernel_counts()
    assert kc["train_fwd_bwd_kernel<mbin>"] == 3 and kc["train_fwd_bwd_kernel"] == 0 and kc["train8_kernel"] == 0, kc
    g.close()


def ref_rollout(ref, seed, E, T, u):
    """runner.hpp:56-157 over the seeded synthetic env with the multi-binary reference policy (the env ignores the actions), the oracle's Normalizer and
    numpy_port.gae.  u [T, E, A] is cleared of near-ties step by step (the observations do not depend on the actions), and returned."""
    from oracle import oracle as o
    from oracle import numpy_port as npp
    nz = o.Normalizer(E, ref.O)
    raw, _, _ = o.seeded_env_step(seed, 0, E, 0, ref.O)
    obs, dones = nz.obs(raw), np.zeros(E, np.float32)
    u = np.array(u, np.float32)
    ro = {k: [] for k in ("obs", "actions", "values", "neglogp", "dones", "rewards")}
    for t in range(T):
        u[t] = clear_uniforms(ref, obs, u[t])
        x, v, nlp, _ = ref.step(obs, u[t])
        for k, val in (("obs", obs), ("actions", x), ("values", v), ("neglogp", nlp), ("dones", dones)):
            ro[k].append(val)
        raw, rew, dones = o.seeded_env_step(seed, 0, E, t + 1, ref.O)
        obs = nz.obs(raw)
        ro["rewards"].append(nz.reward(rew, dones))
    ro = {k: np.array(x) for k, x in ro.items()}
    _, last_v = ref.forward(obs)
    ro["returns"] = npp.gae(ro["rewards"].astype(np.float32), ro["values"].astype(np.float32), ro["dones"], last_v.astype(np.float32), dones, GAMMA, LAM)
    return ro, u


def check_rollout(got, ro, msg):
    np.testing.assert_array_equal(got["actions"], ro["actions"].astype(np.float32), err_msg=msg + " actions")
    for f in ("obs", "values", "neglogp", "rewards", "returns"):
        close(got[f], ro[f], rtol=2e-4, atol=2e-5, msg=msg + " " + f)


FIELDS = ("obs", "actions", "values", "neglogp", "rewards", "returns")


@pytest.mark.gpu
@pytest.mark.parametrize("E,T", [(1, 32), (64, 8), (300, 2)])
def test_collect_synthetic_matches_reference(E, T):
    O, A = 18, 18
    ref, g = make(O, A, (64, 64), seed=E, pi_gain=3.0)
    ro, u = ref_rollout(ref, 1234, E, T, np.random.RandomState(E).uniform(size=(T, E, A)))
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(1234, GAMMA, LAM, u)
    got = {f: g.rollout_get(f) for f in FIELDS}
    assert got["actions"].shape == (T, E, A)
    check_rollout(got, ro, "collect E=%d" % E)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("E,T", [(1, 16), (40, 4), (80, 2)])
def test_host_env_loop_matches_reference(E, T):
    """Up to four row blocks of 16 environments the kernel publishes the sampled rows itself (HF_DIRECT): E = 1 is one live row, E = 40 with A = 7 three blocks of
    [16][7] floats whose last has 8 live rows -- odd elements behind the 16-byte pieces.  E = 80 is five row blocks: the copy form (HF_COPY)."""
    from oracle import oracle as o
    O, A = 18, 7
    ref, g = make(O, A, (64, 64), seed=40 + E, pi_gain=3.0)
    ro, u = ref_rollout(ref, 99, E, T, np.random.RandomState(E + 1).uniform(size=(T, E, A)))
    g.norm_init(E)
    g.rollout_alloc(E, T)
    raw, _, _ = o.seeded_env_step(99, 0, E, 0, O)
    g.rollout_reset(raw)
    acts = []
    for t in range(T):
        a = g.rollout_act(t, u[t])
        assert a.shape == (E, A)
        acts.append(a)
        raw, rew, dn = o.seeded_env_step(99, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    got = {f: g.rollout_get(f) for f in FIELDS}
    np.testing.assert_array_equal(np.array(acts), got["actions"])
    check_rollout(got, ro, "host Env E=%d" % E)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,E,T,nmb", [((64, 64), 32, 16, 4), ((256, 256), 64, 8, 4)])
def test_two_updates_with_explicit_perms_match_reference(hidden, E, T, nmb):
    O, A, epochs = 18, 18, 2
    ref, g = make(O, A, hidden, seed=17, ent_coef=0.01)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    rng = np.random.RandomState(3)
    for it in range(2):
        ro, _ = ref_rollout(ref, 500 + it, E, T, rng.uniform(size=(T, E, A)))
        ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)   # move the ratio off 1
        ref_in = {f: np.asarray(ro[f], np.float32) for f in ("obs", "actions", "values", "neglogp", "returns")}
        for f, x in ref_in.items():
            g.rollout_set(f, x)
        perms = np.stack([rng.permutation(E * T) for _ in range(epochs)]).astype(np.int32)
        rows, mean = g.update(LR, CR, epochs, nmb, perms)
        ref_rows, ref_mean = ref.update(ref_in, perms, nmb, LR, CR)
        close(rows[:, :4], ref_rows[:, :4], rtol=1e-4, atol=1e-6, msg="loss rows update %d" % it)
        assert np.all(np.abs(rows[:, 4] - ref_rows[:, 4]) <= nmb / (E * T) + 1e-6)
        close(mean[:4], ref_mean[:4], rtol=1e-4, atol=1e-6, msg="mean losses update %d" % it)
        close(g.get_flat(0), ref.theta, rtol=1e-4, atol=5e-6, msg="theta after update %d" % it)
        nodes = g.debug_graph_nodes()
        assert nodes is not None and nodes["kernel"] > 0, nodes
        assert nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    g.close()


HEADED = ("policy_step_kernel", "train_fwd_bwd_kernel", "train8_kernel", "narrow_", "bf16_", "weight_grad_assemble")
MINE = ("policy_step_kernel<mbin>", "train_fwd_bwd_kernel<mbin>", "policy_step_kernel<host_action>")


def exercise(hidden, flags):
    """every entry-point family once on a fresh handle; returns its ppo_kernel_counts and a few outputs"""
    from oracle import oracle as o
    E, T, O, A = 64, 4, 18, 18
    ref, g = make(O, A, hidden, seed=1, flags=flags)
    g.norm_init(E)
    g.rollout_alloc(E, T)
    g.collect_synthetic(3, GAMMA, LAM)
    g.update(LR, CR, 1, 4, None, seed=1, want_rows=False)
    raw, _, _ = o.seeded_env_step(5, 0, E, 0, O)
    g.rollout_reset(raw)
    u = np.random.RandomState(0).uniform(size=(T, E, A)).astype(np.float32)
    for t in range(T):
        g.rollout_act(t, u[t])
        raw, rew, dn = o.seeded_env_step(5, 0, E, t + 1, O)
        g.rollout_observe(t, raw, rew, dn)
    g.rollout_finish(GAMMA, LAM)
    bits = g.rollout_get("actions")
    x, v, nlp = g.step(np.zeros((20, O), np.float32), u[0, :20])
    losses = g.train_step(LR, CR, *synth_batch(ref, 64, 1))
    kc = g.kernel_counts()
    out = (bits, x, nlp, losses, g.get_flat(0))
    g.close()
    return kc, out


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [(64, 64), (256, 256)])
def test_kernel_counts_show_the_mbin_variants_only_and_flags_change_nothing(hidden):
    kc, out = exercise(hidden, None)
    assert kc["policy_step_kernel<mbin>"] > 0 and kc["train_fwd_bwd_kernel<mbin>"] > 0, kc
    assert kc["weight_grad_kernel"] > 0 and kc["grad_reduce_kernel"] > 0, kc
    for name, cnt in kc.items():
        if name.startswith(HEADED) and name not in MINE:
            assert cnt == 0, (name, kc)
    assert len(kc) == 60
    for flags in ({"shape_kernels": True}, {"pair_kernels": True}, {"bf16_head": True}):
        kc2, out2 = exercise(hidden, flags)
        assert kc2 == kc, (flags, kc2, kc)
        for a, b in zip(out, out2):
            np.testing.assert_array_equal(a, b, err_msg=str(flags))


@pytest.mark.gpu
def test_errors():
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import PPOConfig
    lib = ppo_cpp_amd.load_library()
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="act_dim >= 1"):
        ppo_cpp_amd.PPOHip(18, 0, [64, 64], action_dist="multi_binary")
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="PPO_BF16"):
        ppo_cpp_amd.PPOHip(18, 6, [256, 256], action_dist="multi_binary", compute_dtype=1)
    cfg = PPOConfig()
    hid = (ctypes.c_int32 * 2)(64, 64)
    lib.ppo_config_default(ctypes.byref(cfg), 18, 6, 2, hid)
    h = ctypes.c_void_p()
    for dist in (2, 3 | 0x1000, 3 | 0x800):
        assert lib.ppo_create_ex(ctypes.byref(cfg), dist, ctypes.byref(h)) != 0
        assert b"unknown action_dist" in lib.ppo_last_error(None)
    ref, g = make(18, 6, (64, 64))
    obs, x, adv, ret, nlp, v = synth_batch(ref, 32, 0)
    theta = g.get_flat(0)
    for bad in (0.5, 2.0, -1.0, np.nan):
        x2 = x.copy(); x2[5, 3] = bad
        with pytest.raises(ppo_cpp_amd.PPOHipError, match="row 5, column 3"):
            g.train_step(LR, CR, obs, x2, adv, ret, nlp, v)
        g.step(obs)                                                 # usable after the error
    np.testing.assert_array_equal(g.get_flat(0), theta)            # nothing was trained
    g.rollout_alloc(4, 8)
    bits = np.zeros((8, 4, 6), np.float32); bits[2, 1, 4] = 0.5
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="row 9, column 4"):
        g.rollout_set("actions", bits)
    mask = np.ones((32, 6), np.float32)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.step(obs, mask=mask)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.act_deterministic(obs, mask=mask)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.train_step(LR, CR, obs, x, adv, ret, nlp, v, mask=mask)
    with pytest.raises(ppo_cpp_amd.PPOHipError, match="action masks need a categorical"):
        g.set_action_masking(True)
    np.testing.assert_array_equal(g.get_flat(0), theta)
    g.train_step(LR, CR, obs, x, adv, ret, nlp, v)
    assert np.abs(g.get_flat(0) - theta).max() > 0
    g.close()


@pytest.mark.gpu
def test_tensor_round_trip_into_a_fresh_handle():
    import ppo_cpp_amd
    ref, g = make(18, 6, (64, 64), seed=4)
    g.train_step(LR, CR, *synth_batch(ref, 64, 2))
    g2 = ppo_cpp_amd.PPOHip(18, 6, [64, 64], action_dist="multi_binary")
    for which in (0, 1, 2):
        g2.set_flat(g.get_flat(which), which)
        np.testing.assert_array_equal(g2.get_flat(which), g.get_flat(which))
    g2.set_beta_powers(g.beta_powers())
    obs = np.random.RandomState(0).uniform(-1, 1, (300, 18)).astype(np.float32)
    np.testing.assert_array_equal(g2.act_deterministic(obs), g.act_deterministic(obs))
    cat = ppo_cpp_amd.PPOHip(18, 6, [64, 64], action_dist="categorical")
    assert cat.P == g.P and [t for t in cat.tensors] == [t for t in g.tensors]        # a categorical handle's tensor list
    gauss = ppo_cpp_amd.PPOHip(18, 6, [64, 64])
    assert gauss.P == g.P + 6
    for h in (g, g2, cat, gauss):
        h.close()


@pytest.mark.gpu
def test_ppo2_checkpoint_of_a_multi_binary_policy(tmp_path):
    """PPO2::save writes "action_binary": true and 14 model tensors (no pi/logstd); PPO2::load into a fresh multi-binary handle restores every tensor (same
    deterministic actions); into a categorical handle of the same width it is refused, and so is a categorical checkpoint into the multi-binary handle"""
    import json
    from ppo_cpp_amd import hostapi
    prefix = str(tmp_path / "mbin")
    obs = np.random.RandomState(3).uniform(-1, 1, (200, 18)).astype(np.float32)
    rc, before, after = hostapi.binary_checkpoint(prefix, obs)
    assert rc == 0, rc
    np.testing.assert_array_equal(before, after)
    assert before.shape == (200, 6) and set(np.unique(before)) <= {0.0, 1.0} and before.any() and not before.all()
    side = json.load(open(prefix + ".json"))
    assert side["action_binary"] is True and side["action_space"] == "discrete" and "action_nvec" not in side
    assert "action_binary" not in json.load(open(prefix + ".cat.json"))
    lib = hostapi.load_host_library()
    buf = np.zeros(64 * 64, np.float32); shape = (ctypes.c_longlong * 4)()
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.ppo_host_bundle_tensor(prefix.encode(), b"model/pi/logstd", fp, buf.size, shape) == -2
    model = ["pi_fc0/w", "pi_fc0/b", "vf_fc0/w", "vf_fc0/b", "pi_fc1/w", "pi_fc1/b", "vf_fc1/w", "vf_fc1/b", "vf/w", "vf/b", "pi/w", "pi/b", "q/w", "q/b"]
    assert len(model) == 14
    for name in model:
        assert lib.ppo_host_bundle_tensor(prefix.encode(), ("model/" + name).encode(), fp, buf.size, shape) > 0, name
    assert lib.ppo_host_bundle_tensor(prefix.encode(), b"model/pi/w", fp, buf.size, shape) == 64 * 6 and list(shape)[:2] == [64, 6]


@pytest.mark.gpu
def test_two_ranks_global_shuffle_equal_one_rank_over_the_union(tmp_path):
    """world 2 on the collective-library stand-in (two processes on one GPU, tests/fake_rccl), ppo_dist_global_shuffle(1): the rollout's action rows travel through
    the all-gather A floats wide, and the weights after one update equal a one-rank update over the union of the rows (the flow and the tolerance of
    tests/test_discrete_policy.py's test of this name)"""
    import subprocess
    import sys
    from tests.test_dp_two_ranks import build_fake_rccl
    world, hidden, E, T, nmb, epochs, A = 2, (64, 64), 32, 8, 4, 2, 6
    tmp = str(tmp_path)
    fake = build_fake_rccl(tmp)
    ref, g = make(18, A, hidden, seed=21)
    rng = np.random.RandomState(8)
    ro, _ = ref_rollout(ref, 77, E, T, rng.uniform(size=(T, E, A)))
    ro = {f: np.asarray(ro[f], np.float32) for f in ("obs", "actions", "values", "neglogp", "returns")}
    ro["neglogp"] = (ro["neglogp"] + rng.normal(scale=0.1, size=(T, E))).astype(np.float32)
    gperms = np.stack([rng.permutation(E * T).astype(np.int32) for _ in range(epochs)])
    theta0 = ref.theta.astype(np.float32)
    uid = np.zeros(128, np.uint8)
    name = ("/ppo_dp_mbin_%d_%d" % (os.getpid(), rng.randint(1 << 30))).encode()
    uid[:len(name)] = np.frombuffer(name, np.uint8)
    fin = os.path.join(tmp, "in.npz")
    np.savez(fin, hidden=np.array(hidden), E=E, T=T, nmb=nmb, epochs=epochs, A=A, theta=theta0, uid=uid, gperms=gperms, lr=LR, cr=CR,
             **{"ro_" + f: x for f, x in ro.items()})
    env = dict(os.environ, PPO_RCCL_LIBRARY=fake, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker_multi_binary.py"), str(r), str(world), fin, os.path.join(tmp, "out%d.npz" % r)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=300)[0].decode())
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("data-parallel workers timed out")
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    outs = [np.load(os.path.join(tmp, "out%d.npz" % r)) for r in range(world)]
    g.norm_init(E, 0.99)
    g.rollout_alloc(E, T)
    for f, x in ro.items():
        g.rollout_set(f, x)
    rows, _ = g.update(LR, CR, epochs, nmb, gperms)
    theta1 = g.get_flat(0)
    g.close()
    for r, out in enumerate(outs):
        np.testing.assert_array_equal(out["actions"], ro["actions"][:, r * (E // world):(r + 1) * (E // world)])
        close(out["rows"][:, :4], rows[:, :4], rtol=2e-4, atol=2e-6, msg="loss rows rank %d" % r)
        close(out["theta"], theta1, rtol=2e-4, atol=5e-6, msg="weights rank %d" % r)
    for k in ("rows", "theta", "adam_m", "adam_v"):
        np.testing.assert_array_equal(outs[0][k], outs[1][k])
    assert np.abs(theta1 - theta0).max() > 0


LEARN_UPDATES = 600


@pytest.mark.gpu
def test_ppo2_learns_the_multi_binary_target_task():
    """Learning: MultiBinaryTargetEnv x 16 (host/env/env_mock.hpp: 18 bits, reward = the share of bits with x_j == ((W obs)_j > 0) with TargetEnv's W, episodes of
    100 steps) behind VecEnv + EnvNormalize, 64 steps, [64,64], 600 updates of 4 epochs x 4 minibatches at lr 2e-3, cliprange 0.2, through PPO2::learn with the
    library's own sampling and shuffles.  A uniform policy earns 0.5.  Eighteen bits share one reward, so the curve rises slowly: N was raised from 60 in steps (60,
    100, .. 500, 525, 550, 575, 600) until the NumPy reference loop (tests/bernoulli_ref.reference_curve: BernRef.learn_loop on MultiBinaryTargetRef(1234, 16, 18, 18)
    with the oracle's EnvNormalize, measured on the CPU) rose by at least 0.15 on each of three draw seeds -- first-15 -> last-15 mean reward
    0.509 -> 0.662, 0.506 -> 0.672, 0.506 -> 0.658 (rises 0.152, 0.166, 0.151; at 575 updates 0.145, 0.159, 0.153).
    RISE = 0.09: the last-15 mean over the first-15, 0.6 x the smallest reference rise (0.151).
    BAND = 0.06: |last-15 mean - 0.664| (the reference's mean over the seeds), four times the seeds' spread of 0.0146 and not below 0.05; the two legs differ in
    initial weights and draws.  The proportions of tests/test_discrete_policy.py's learning test.
    This leg on an MI355X: 0.501 -> 0.673 (rise 0.172; 0.009 from the reference's mean), 1.6 s."""
    from ppo_cpp_amd import hostapi
    RISE, BAND, REF_LAST15 = 0.09, 0.06, 0.664
    got = hostapi.learn_curve(16, 64, [64, 64], LEARN_UPDATES, 4, 4, 2e-3, 0.2, act_dim=18, binary=True)
    c = got["reward_curve"]
    first, last = c[:15].mean(), c[-15:].mean()
    print("reward curve first-15 %.3f last-15 %.3f" % (first, last))
    kc = got["kernel_counts"]
    assert kc["policy_step_kernel<mbin>"] > 0 and kc["train_fwd_bwd_kernel<mbin>"] > 0 and kc["policy_step_kernel"] == 0 and kc["train_fwd_bwd_kernel"] == 0, kc
    assert abs(first - 0.5) <= 0.03, first
    assert last - first >= RISE, (first, last)
    assert abs(last - REF_LAST15) <= BAND, (last, REF_LAST15)
