"""Querying the policy: ppo_evaluate_actions, ppo_action_probability, ppo_rollout_evaluate (policy_eval_kernel) and the host layer above them.

Float64 arbiters: the oracle for the Gaussian head, CatRef / MaskedCatRef / MultiCatRef / BernRef with head_edges_ref.head_stats / neglogp_of / entropy_of for the
discrete ones.  `close` is the project's act tolerance (rtol 1e-4, atol 1e-5).  The probability bound is that tolerance on log p carried over to p:
    |p - p_ref| <= 2 p_ref (1e-5 + 1e-4 |log p_ref|) + 1e-37
(d p = p d log p; the factor 2 covers the second-order term of exp and the share of the normaliser; 1e-37 sits at the edge of the float32 normal range, where a
probability that float64 still resolves has become 0 or a denormal in float32)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import head_edges_ref as E
from tests.bernoulli_ref import BernRef, bern_stats, emulate_f32
from tests.masked_categorical_ref import MaskedCatRef, random_masks
from tests.multi_categorical_ref import MultiCatRef, offsets
from tests.multi_categorical_ref import random_masks as multi_random_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 3, (4, 5)), (18, 6, (64, 64)), (18, 18, (256, 256)), (50, 40, (256, 256)), (256, 64, (1024, 1024))]     # one per rung of the ladder
SHAPE_IDS = ["%d-%d-%s" % (O, A, "x".join(map(str, h))) for O, A, h in SHAPES]
ROWS = (1, 17, 300)                                                                                                    # a partial last tile included
NVEC = {3: (3,), 6: (4, 2), 18: (6, 6, 6), 40: (17, 3, 20), 64: (20, 2, 17, 25)}        # a split of A (every component needs two categories: 3 stays whole)
HEADS = ("gaussian", "categorical", "categorical_masked", "multi", "multi_masked", "multi_binary")
HALF_LOG_2PIE = 0.5 * np.log(2.0 * np.pi * np.e)


def close(a, b, msg=""):
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5, err_msg=msg)


def prob_bound(p_ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.where(p_ref > 0, np.abs(np.log(np.where(p_ref > 0, p_ref, 1.0))), 0.0)
    return 2.0 * p_ref * (1e-5 + 1e-4 * lg) + 1e-37


# ---- not GPU ----------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_and_the_host_layer_carries_the_methods():
    import ppo_cpp_amd
    hdr = open(os.path.join(ROOT, "include", "ppo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ppo_cpp_amd.load_library()
    for s in ("ppo_distribution_width", "ppo_evaluate_actions", "ppo_action_probability", "ppo_rollout_evaluate"):
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
        assert hasattr(lib, s), s
    assert re.search(r"#define\s+PPO_ABI_VERSION\s+3\b", hdr) and lib.ppo_abi_version() == 3
    pol = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "ppo2", "policies.hpp")).read()
    assert re.search(r"std::vector<Mat>\s+evaluate_actions\s*\(", pol) and re.search(r"Mat\s+proba_step\s*\(", pol)
    ppo2 = open(os.path.join(ROOT, "ppo_cpp_amd", "host", "ppo2", "ppo2.hpp")).read()
    assert re.search(r"Mat\s+action_probability\s*\(const Mat& obs, const Mat\* actions = nullptr, bool logp = false, const Mat\* mask = nullptr\)", ppo2)
    assert "ppo_host_policy_query" in open(os.path.join(ROOT, "ppo_cpp_amd", "host", "ppo_host.cpp")).read()
    for name in ("evaluate_actions", "action_probability", "distribution_width", "rollout_evaluate"):
        assert hasattr(ppo_cpp_amd.PPOHip, name), name


def softmax_f32(logits):
    """the kernel's statement in float32: m = max, ex_j = exp(l_j - m), z = the SEQUENTIAL float32 sum of ex, p_j = ex_j / z"""
    f = np.float32
    l = np.asarray(logits, f)
    ex = np.exp(l - l.max(axis=1, keepdims=True), dtype=f)
    z = np.zeros(len(l), f)
    for j in range(l.shape[1]):
        z = (z + ex[:, j]).astype(f)
    return (ex / z[:, None]).astype(f)


@pytest.mark.parametrize("spread", [1.5, 40.0, 120.0])
@pytest.mark.parametrize("width", [2, 6, 40, 70])
def test_float32_statement_of_the_probabilities_stays_inside_the_bound(spread, width):
    rng = np.random.RandomState(int(spread) * 100 + width)
    l = (spread * rng.uniform(-1, 1, (4096, width))).astype(np.float32)
    p_ref = E.head_stats([width], l.astype(np.float64))[0][2]
    p = softmax_f32(l).astype(np.float64)
    worst = float((np.abs(p - p_ref) / prob_bound(p_ref)).max())
    sums = float(np.abs(p.sum(axis=1) - 1.0).max())
    print("softmax spread %g width %d: %.2f %% of the bound, row sums within %.2g" % (spread, width, 100 * worst, sums))
    assert worst <= 1.0 and sums <= 2e-6
    b_ref = bern_stats(l)[0]
    b = emulate_f32(l, x=np.zeros_like(l))[0].astype(np.float64)
    worst_b = float((np.abs(b - b_ref) / prob_bound(b_ref)).max())
    print("sigmoid spread %g width %d: %.2f %% of the bound" % (spread, width, 100 * worst_b))
    assert worst_b <= 1.0 and np.isfinite(b).all()


# ---- handles and references ----------------------------------------------------------------------------------------------------------------------------------
def kind_of(head):
    return "multi_binary" if head == "multi_binary" else head.split("_")[0]


def nvec_of(head, A):
    return list(NVEC[A]) if kind_of(head) == "multi" else [A]


def make(head, O, A, hidden, **kw):
    """(float64 reference, handle)"""
    import ppo_cpp_amd
    from oracle import oracle as o
    k = kind_of(head)
    if k == "gaussian":
        return o.Oracle(O, A, list(hidden)), ppo_cpp_amd.PPOHip(O, A, list(hidden), **kw)
    if k == "categorical":
        return MaskedCatRef(O, A, hidden), ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="categorical", **kw)
    if k == "multi":
        return MultiCatRef(O, NVEC[A], hidden), ppo_cpp_amd.PPOHip(O, None, list(hidden), action_dist="multi_categorical", nvec=NVEC[A], **kw)
    return BernRef(O, A, hidden), ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="multi_binary", **kw)


def set_weights(head, ref, g, seed, pi_gain=1.0, bias=None):
    """random weights with the head's gain `pi_gain`, or (bias given) pi/w = 0 and pi/b = bias: every row's logits are `bias` bit for bit"""
    if kind_of(head) == "gaussian":
        ref.init_orthogonal(seed)
        ref.tensor("pi/w")[:] *= np.float32(pi_gain / 0.01)            # (init_orthogonal's head gain is 0.01)
        ref.tensor("pi/logstd")[:] = np.random.RandomState(seed + 1).uniform(-1.0, 0.2, (1, ref.A))
    elif bias is None:
        ref.init_random(seed, pi_gain)
    else:
        E.exact_theta(ref, seed, bias)
    g.set_flat(ref.theta)


def masks_for(head, rng, n, A):
    if not head.endswith("_masked"):
        return None
    return multi_random_masks(rng, n, NVEC[A]) if kind_of(head) == "multi" else random_masks(rng, n, A)


def random_actions(head, rng, n, A, mask):
    """valid actions the policy did not draw: any allowed category per component, any bit"""
    k = kind_of(head)
    if k == "multi_binary":
        return (rng.uniform(size=(n, A)) < 0.5).astype(np.float32)
    nvec = nvec_of(head, A)
    off = offsets(nvec)
    acts = np.zeros((n, len(nvec)), np.float32)
    for c, nk in enumerate(nvec):
        score = rng.uniform(size=(n, nk))
        if mask is not None:
            score = np.where(mask[:, off[c]:off[c + 1]] != 0, score, -1.0)
        acts[:, c] = np.argmax(score, axis=1)
    return acts if k == "multi" else acts[:, 0]


def reference(head, ref, obs, acts, mask, noise=None):
    """float64 (value, neglogp of acts, entropy, parameters [n, W]); the Gaussian's actions are the oracle's own draw under `noise`"""
    k = kind_of(head)
    if k == "gaussian":
        a, v, nlp = ref.step(obs, noise)
        mu, _ = ref.forward(obs)
        ls = ref.tensor("pi/logstd").astype(np.float64).reshape(-1)
        ent = np.full(len(obs), (ls + HALF_LOG_2PIE).sum())
        return a, v, nlp, ent, np.concatenate([mu.astype(np.float64), np.broadcast_to(np.exp(ls), mu.shape)], axis=1)
    logits, v = ref.forward(obs)
    if k == "multi_binary":
        p, nlp1, nlp0, ent = bern_stats(logits)
        return acts, v, np.where(acts > 0, nlp1, nlp0).sum(axis=1), ent.sum(axis=1), p
    nvec = nvec_of(head, ref.A)
    p = np.concatenate([s[2] for s in E.head_stats(nvec, logits, mask)], axis=1)
    return acts, v, E.neglogp_of(nvec, logits, acts, mask), E.entropy_of(nvec, logits, mask), p


def check_params(head, g, ref, obs, mask, got, want, tag):
    k = kind_of(head)
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), tag
    if k == "gaussian":
        close(got, want, tag + " mu | std")
        return
    p = got.astype(np.float64)
    over = np.abs(p - want) / prob_bound(want)
    assert over.max() <= 1.0, "%s: probability %.3g of the bound at %s" % (tag, over.max(), np.unravel_index(over.argmax(), over.shape))
    logits = ref.forward(obs)[0]
    if k == "multi_binary":
        sure = np.abs(logits) > E.TIE
        np.testing.assert_array_equal((got > 0.5)[sure], (g.act_deterministic(obs) > 0)[sure], tag + " mode")
        return
    nvec = nvec_of(head, ref.A)
    off = offsets(nvec)
    if mask is not None:
        forb = got[mask == 0]
        assert (forb == 0).all() and not np.signbit(forb).any(), tag + ": a forbidden category's probability is exactly +0"
    det = g.act_deterministic(obs, mask=mask).reshape(len(obs), len(nvec))
    sure = E.top2_gap(nvec, logits if mask is None else np.where(mask != 0, logits, -np.inf)) > E.TIE
    for c in range(len(nvec)):
        pc = got[:, off[c]:off[c + 1]]
        assert np.abs(pc.astype(np.float64).sum(axis=1) - 1.0).max() <= 2e-6, tag + " component sum"
        np.testing.assert_array_equal(np.argmax(pc, axis=1)[sure[:, c]], det[sure[:, c], c], tag + " argmax")


def weight_cases(head, A):
    """(name, pi_gain, bias): random, peaked random, and logits written into pi/b -- rows of head_edges_ref.logit_table, +-40 and +-120 for the bits"""
    out = [("random", 1.0, None), ("gain3", 3.0, None)]
    k = kind_of(head)
    if k == "multi_binary":
        sign = np.where(np.arange(A) % 2 == 0, 1.0, -1.0)
        out += [("bits40", 1.0, 40.0 * sign), ("bits120", 1.0, -120.0 * sign)]
    elif k != "gaussian":
        table, _ = E.logit_table(nvec_of(head, A))
        out += [(c, 1.0, table[c]) for c in ("peaked40", "peaked120", "forbidden_high")]
    return out


# ---- 3: against float64 --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("O,A,hidden", SHAPES, ids=SHAPE_IDS)
def test_queries_match_float64(O, A, hidden, head):
    ref, g = make(head, O, A, hidden)
    assert g.distribution_width == (2 * A if head == "gaussian" else A)
    for wi, (name, gain, bias) in enumerate(weight_cases(head, A)):
        set_weights(head, ref, g, 11 + wi, gain, bias)
        for n in ROWS:
            rng = np.random.RandomState(100 * wi + n)
            obs = rng.uniform(-2, 2, (n, O)).astype(np.float32)
            mask = masks_for(head, rng, n, A)
            if mask is not None and name == "forbidden_high":
                mask[0] = (~E.logit_table(nvec_of(head, A))[1]).astype(np.float32)      # the pattern the row is written for: every high logit forbidden
            noise = rng.normal(size=(n, A)).astype(np.float32)
            acts, rv, rnlp, rent, rpar = reference(head, ref, obs, None if head == "gaussian" else random_actions(head, rng, n, A, mask), mask, noise)
            tag = "%s %s n=%d" % (head, name, n)
            v, nlp, ent = g.evaluate_actions(obs, acts, mask)
            for x in (v, nlp, ent):
                assert x.shape == (n,) and np.isfinite(x).all(), tag
            close(v, rv, tag + " value"); close(nlp, rnlp, tag + " neglogp"); close(ent, rent, tag + " entropy")
            check_params(head, g, ref, obs, mask, g.action_probability(obs, mask), rpar, tag)


# ---- 4: the act model's bits -----------------------------------------------------------------------------------------------------------------------------------
def step_family(g):
    """'generic' when the handle's steps ran policy_step_kernel, 'narrow' when narrow_step_kernel or a one-launch form did"""
    kc = {k: v for k, v in g.kernel_counts().items() if v}
    assert any(k.startswith(("policy_step_kernel", "narrow_step_kernel")) for k in kc), kc
    return "generic" if any(k.startswith("policy_step_kernel") for k in kc) else "narrow"


def act_model_roundtrip(head, g, ref, O, A, n, exact, seed=3):
    rng = np.random.RandomState(seed)
    set_weights(head, ref, g, seed, 1.0)
    obs = rng.uniform(-2, 2, (n, O)).astype(np.float32)
    mask = masks_for(head, rng, n, A)
    noise = (rng.normal(size=(n, A)) if head == "gaussian" else np.clip(rng.uniform(size=(n, A)), 1e-6, 1 - 1e-6)).astype(np.float32)
    a, v, nlp = g.step(obs, noise, mask=mask)
    same = np.testing.assert_array_equal if exact else close
    assert step_family(g) == ("generic" if exact else "narrow")
    v2, nlp2, ent = g.evaluate_actions(obs, a, mask)
    same(nlp2, nlp, "neglogp of the drawn action"); same(v2, v, "value"); same(v2, g.value(obs), "ppo_value")
    if head == "gaussian":
        same(g.action_probability(obs)[:, :A], g.act_deterministic(obs), "mu")


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("O,A,hidden", SHAPES, ids=SHAPE_IDS)
def test_bits_of_the_act_model_on_generic_family_handles(O, A, hidden, head, monkeypatch):
    if head == "gaussian":
        monkeypatch.setenv("PPO_HIP_NO_NARROW", "1")                   # (read at creation: the [64,64] and [4,5] Gaussian handles then step with policy_step_kernel)
    ref, g = make(head, O, A, hidden)
    for n in (17, 300):
        act_model_roundtrip(head, g, ref, O, A, n, exact=True)


@pytest.mark.gpu
@pytest.mark.parametrize("head", ["gaussian", "categorical", "categorical_masked", "multi", "multi_masked"])
def test_narrow_family_handles_agree_to_rounding(head):
    ref, g = make(head, 18, 6, (64, 64), **({} if head == "gaussian" else {"shape_kernels": True}))
    act_model_roundtrip(head, g, ref, 18, 6, 300, exact=False)


# ---- 5: entropy ties to training ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("O,A,hidden", [(18, 6, (64, 64)), (18, 18, (256, 256))], ids=["18-6-64x64", "18-18-256x256"])
def test_mean_entropy_is_the_train_steps_entropy_loss(O, A, hidden, head):
    ref, g = make(head, O, A, hidden)
    set_weights(head, ref, g, 5, 3.0)
    rng = np.random.RandomState(9)
    n = 64
    obs = rng.uniform(-2, 2, (n, O)).astype(np.float32)
    mask = masks_for(head, rng, n, A)
    noise = (rng.normal(size=(n, A)) if head == "gaussian" else np.clip(rng.uniform(size=(n, A)), 1e-6, 1 - 1e-6)).astype(np.float32)
    a, v, nlp = g.step(obs, noise, mask=mask)
    _, _, ent = g.evaluate_actions(obs, a, mask)                       # the query first: the train step moves the weights
    advs = rng.normal(size=n).astype(np.float32)
    losses = g.train_step(E.LR, E.CR, obs, a, advs, (v + 0.1 * rng.normal(size=n)).astype(np.float32), nlp, v, mask=mask)
    np.testing.assert_allclose(ent.astype(np.float64).mean(), losses[2], rtol=1e-4, atol=1e-6)


# ---- 6: statelessness --------------------------------------------------------------------------------------------------------------------------------------------
def all_queries(g, obs, acts, mask=None, rollout=True):
    out = [g.evaluate_actions(obs, acts, mask), g.action_probability(obs, mask)]
    if rollout:
        out.append(g.rollout_evaluate())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("head", ["gaussian", "categorical", "multi_binary"])
def test_queries_leave_draws_counts_weights_and_adam_state_alone(head):
    O, A, hidden = 18, 6, (64, 64)
    ref, g = make(head, O, A, hidden)
    set_weights(head, ref, g, 2)
    rng = np.random.RandomState(4)
    obs = rng.uniform(-2, 2, (33, O)).astype(np.float32)
    g.rollout_alloc(4, 8)
    g.collect_synthetic(3, 0.99, 0.95)
    acts = g.step(obs)[0]
    g.seed(7)
    plain = [g.step(obs) for _ in range(3)]
    before = (g.kernel_counts(), [g.get_flat(w) for w in range(3)], g.beta_powers())
    all_queries(g, obs, acts)
    after = (g.kernel_counts(), [g.get_flat(w) for w in range(3)], g.beta_powers())
    assert before[0] == after[0] and len(after[0]) == 60
    for x, y in zip(before[1] + [before[2]], after[1] + [after[2]]):
        np.testing.assert_array_equal(x, y)
    g.seed(7)
    mixed = []
    for _ in range(3):
        all_queries(g, obs, acts)
        mixed.append(g.step(obs))
        all_queries(g, obs, acts)
    for p, m in zip(plain, mixed):
        for x, y in zip(p, m):
            np.testing.assert_array_equal(x, y)


FIELDS = ("obs", "actions", "values", "neglogp", "dones", "rewards", "returns")


def gaussian_6464(seed=2):
    ref, g = make("gaussian", 18, 18, (64, 64))
    set_weights("gaussian", ref, g, seed)
    g.seed(5)
    return g


@pytest.mark.gpu
def test_queries_between_collects_and_inside_a_host_env_rollout_change_nothing():
    E_, T = 4, 8
    rng = np.random.RandomState(1)
    qobs = rng.uniform(-2, 2, (19, 18)).astype(np.float32)
    qact = rng.normal(size=(19, 18)).astype(np.float32)
    raw = rng.uniform(-3, 3, (T + 1, E_, 18)).astype(np.float32)
    rew = rng.normal(size=(T, E_)).astype(np.float32)
    dones = (rng.uniform(size=(T, E_)) < 0.2).astype(np.float32)
    got = []
    for query in (False, True):
        g = gaussian_6464()
        g.rollout_alloc(E_, T)
        g.collect_synthetic(3, 0.99, 0.95)
        if query:
            all_queries(g, qobs, qact)
        g.collect_synthetic(3, 0.99, 0.95, step0=T, first=False)
        out = {"synthetic/" + f: g.rollout_get(f) for f in FIELDS}
        g.rollout_reset(raw[0])                                        # a host Env: a query between every act and observe, and between observe and the next act
        for t in range(T):
            a = g.rollout_act(t)
            if query:
                all_queries(g, qobs, qact, rollout=False)
                with pytest.raises(Exception, match="not finished"):
                    g.rollout_evaluate()
            g.rollout_observe(t, raw[t + 1], rew[t], dones[t])
            if query:
                all_queries(g, qobs, qact, rollout=False)
            out["host/act%d" % t] = a
        g.rollout_finish(0.99, 0.95)
        out.update({"host/" + f: g.rollout_get(f) for f in FIELDS})
        got.append(out)
    # (kernel_counts is not compared here: a query in the middle of a resident rollout retires and relaunches the resident kernel, as ppo_value does, and every
    # launch of that kernel is counted)
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], k)


@pytest.mark.gpu
def test_queries_see_the_weights_of_a_deferred_adam_update():
    g = gaussian_6464()
    g.rollout_alloc(4, 8)
    g.collect_synthetic(3, 0.99, 0.95)
    g.update(E.LR, E.CR, 2, 2, seed=1)
    obs = g.rollout_get("obs").reshape(-1, 18)
    v, _, _ = g.evaluate_actions(obs, g.rollout_get("actions").reshape(-1, 18))
    close(v, g.value(obs), "value under the updated weights")
    assert np.abs(v - g.rollout_get("values").reshape(-1)).max() > 0          # the update moved the value tower


# ---- 7: the device-resident rollout -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("E_,T", [(8, 4), (40, 3)])
@pytest.mark.parametrize("head,hidden", [("gaussian", (64, 64)), ("gaussian", (256, 256)), ("categorical", (64, 64)), ("categorical_masked", (64, 64)),
                                         ("multi", (256, 256)), ("multi_masked", (64, 64)), ("multi_binary", (64, 64))])
def test_rollout_evaluate(head, hidden, E_, T):
    O, A = 18, 18
    ref, g = make(head, O, A, hidden)
    set_weights(head, ref, g, 6, 2.0)
    with pytest.raises(Exception, match="no rollout allocated"):
        g.rollout_evaluate()
    if head.endswith("_masked"):
        g.set_action_masking(True)
    g.rollout_alloc(E_, T)
    with pytest.raises(Exception, match="not finished"):
        g.rollout_evaluate()
    g.collect_synthetic(3, 0.99, 0.95)
    v, nlp, ent = g.rollout_evaluate()
    narrow = any(k.startswith("narrow") and c for k, c in g.kernel_counts().items())
    assert narrow == (head == "gaussian" and hidden == (64, 64))
    same = close if narrow else np.testing.assert_array_equal
    same(nlp, g.rollout_get("neglogp"), "field 3"); same(v, g.rollout_get("values"), "field 2")
    assert ent.shape == (T, E_) and np.isfinite(ent).all()
    g.update(E.LR, E.CR, 1, 1, seed=1)
    v, nlp, ent = g.rollout_evaluate()
    obs, acts = g.rollout_get("obs").reshape(-1, O), g.rollout_get("actions")
    mask = g.rollout_get("masks").reshape(-1, A) if head.endswith("_masked") else None
    v2, nlp2, ent2 = g.evaluate_actions(obs, acts.reshape((E_ * T,) + acts.shape[2:]), mask)
    for x, y in ((v, v2), (nlp, nlp2), (ent, ent2)):
        np.testing.assert_array_equal(x.reshape(-1), y)
    assert np.abs(nlp - g.rollout_get("neglogp")).max() > 0                   # the update moved the policy
    g.rollout_reset(np.zeros((E_, O), np.float32))
    g.rollout_act(0)
    with pytest.raises(Exception, match="not finished"):
        g.rollout_evaluate()


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def fp(x):
    return x.ctypes.data_as(C.POINTER(C.c_float))


@pytest.mark.gpu
def test_refusals_leave_the_handle_usable():
    import ppo_cpp_amd
    rng = np.random.RandomState(0)
    n = 5
    obs = rng.uniform(-1, 1, (n, 18)).astype(np.float32)
    ones = np.ones((n, 6), np.float32)

    def refused(g, match, f):
        kc = g.kernel_counts()
        with pytest.raises(ppo_cpp_amd.PPOHipError, match=match):
            f()
        assert g.kernel_counts() == kc

    b = ppo_cpp_amd.PPOHip(256, 64, [1024, 1024], compute_dtype=1)
    b.init_orthogonal(0)
    bobs = rng.uniform(-1, 1, (n, 256)).astype(np.float32)
    refused(b, "PPO_BF16", lambda: b.evaluate_actions(bobs, np.zeros((n, 64), np.float32)))
    refused(b, "PPO_BF16", lambda: b.action_probability(bobs))
    refused(b, "PPO_BF16", lambda: b.rollout_evaluate())
    assert np.isfinite(b.value(bobs)).all()

    for head in ("gaussian", "multi_binary"):
        _, g = make(head, 18, 6, (64, 64))
        g.init_orthogonal(0)
        acts = np.zeros((n, 6), np.float32)
        refused(g, "action masks need a categorical", lambda: g.evaluate_actions(obs, acts, ones))
        refused(g, "action masks need a categorical", lambda: g.action_probability(obs, ones))
        if head == "multi_binary":
            for bad in (0.5, 2.0, np.nan):
                x = acts.copy(); x[3, 2] = bad
                refused(g, "row 3, column 2.*not 0 or 1", lambda: g.evaluate_actions(obs, x))
        assert np.isfinite(g.evaluate_actions(obs, acts)[1]).all()

    _, g = make("categorical", 18, 6, (64, 64))
    g.init_orthogonal(0)
    kc0 = g.kernel_counts()
    acts = np.zeros(n, np.float32)
    for bad in (6.0, -1.0, 2.5, np.nan):
        x = acts.copy(); x[2] = bad
        refused(g, r"actions\[2\].*not a category index in \[0, 6\)", lambda: g.evaluate_actions(obs, x))
    m = ones.copy(); m[1, 0] = 0
    refused(g, r"actions\[1\] = 0 is forbidden by the row's own mask", lambda: g.evaluate_actions(obs, acts, m))
    m = ones.copy(); m[4] = 0
    refused(g, "mask row 4 allows no category", lambda: g.evaluate_actions(obs, np.ones(n, np.float32), m))
    refused(g, "mask row 4 allows no category", lambda: g.action_probability(obs, m))
    refused(g, "n must be positive", lambda: g.evaluate_actions(obs[:0], acts[:0]))
    refused(g, "n must be positive", lambda: g.action_probability(obs[:0]))
    out = np.zeros(n, np.float32)
    lib = g.lib
    assert lib.ppo_evaluate_actions(g.h, fp(obs), fp(acts), n, None, None, None, None) != 0 and b"all NULL" in lib.ppo_last_error(g.h)
    assert lib.ppo_rollout_evaluate(g.h, None, None, None) != 0 and b"all NULL" in lib.ppo_last_error(g.h)
    par = np.zeros((n, 6), np.float32)
    assert lib.ppo_action_probability(g.h, fp(obs), n, None, fp(par), C.c_int64(n * 6 + 1)) != 0 and b"is not n * W" in lib.ppo_last_error(g.h)
    assert lib.ppo_evaluate_actions(g.h, fp(obs), fp(acts), n, None, None, fp(out), None) == 0 and np.isfinite(out).all()      # one output alone is a call
    assert g.kernel_counts() == kc0

    _, g = make("multi", 18, 6, (64, 64))
    g.init_orthogonal(0)
    acts = np.zeros((n, 2), np.float32)
    x = acts.copy(); x[2, 1] = 2.0
    refused(g, r"row 2, component 1: action 2 is not a category index in \[0, 2\)", lambda: g.evaluate_actions(obs, x))
    m = ones.copy(); m[3, 4:] = 0
    refused(g, "mask row 3 allows no category of component 1", lambda: g.evaluate_actions(obs, acts, m))
    m = ones.copy(); m[3, 4] = 0
    refused(g, "row 3, component 1: action 0 is forbidden", lambda: g.evaluate_actions(obs, acts, m))
    assert np.isfinite(g.evaluate_actions(obs, acts, ones)[1]).all()


# ---- 9: host layer -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("head", ["gaussian", "categorical_masked", "multi"])
def test_host_layer_returns_the_c_abis_bits(head):
    from ppo_cpp_amd import hostapi
    O, A, hidden, n = 18, 6, (64, 64), 37
    ref, g = make(head, O, A, hidden)
    set_weights(head, ref, g, 8, 2.0)
    rng = np.random.RandomState(2)
    obs = rng.uniform(-2, 2, (n, O)).astype(np.float32)
    mask = masks_for(head, rng, n, A)
    acts = rng.normal(size=(n, A)).astype(np.float32) if head == "gaussian" else random_actions(head, rng, n, A, mask)
    v, nlp, ent = g.evaluate_actions(obs, acts, mask)
    q = hostapi.policy_query(g, obs, acts, mask)
    np.testing.assert_array_equal(q["values"], v); np.testing.assert_array_equal(q["neglogps"], nlp); np.testing.assert_array_equal(q["entropies"], ent)
    np.testing.assert_array_equal(q["params"], g.action_probability(obs, mask))
    np.testing.assert_array_equal(q["logprob"], -nlp)
    np.testing.assert_allclose(q["prob"], np.exp(-nlp.astype(np.float64)), rtol=1e-6, atol=1e-44)
