"""The policy queries of a PPO_BF16 handle (ppo_set_bf16_queries: bf16_eval_kernel) at 20 observations, hidden [128, 128].  Tolerances against float64 are those of
tests/test_policy_query.py (close, prob_bound, component sums within 2e-6).  "The fp32 exp(logstd)" is the device's expf: the std a PPO_F32 handle's query returns."""
import numpy as np
import pytest
from tests import bf16_ref as R, head_edges_ref as E
from tests.multi_categorical_ref import MultiCatRef, offsets, random_masks
from tests.test_policy_query import HALF_LOG_2PIE, close, prob_bound, set_weights

pytestmark = pytest.mark.gpu
# rows: a lone one, a partial block, past the 128-row pad; 70 actions: lanes own a second element; (3, 70, 5): the middle component straddles lanes 63 / 64
O, HIDDEN, ROWS = 20, (128, 128), (1, 5, 130)
HEADS = {"gauss6": (6,), "gauss70": (70,), "cat6": (6,), "cat6_masked": (6,), "cat128": (128,), "cat128_masked": (128,), "multi": (3, 70, 5), "multi_masked": (3, 70, 5)}


def make(head, dtype=1, on=True, **kw):
    import ppo_cpp_amd                                         # -> (float64 reference, handle); MultiCatRef serves the categorical head as its one-component form
    from oracle import oracle as o
    nvec, gauss = HEADS[head], head.startswith("gauss")
    ref = o.Oracle(O, nvec[0], list(HIDDEN)) if gauss else MultiCatRef(O, nvec, HIDDEN)
    dist = {} if gauss else dict(action_dist="categorical", bf16_head=True) if head.startswith("cat") else dict(action_dist="multi_categorical", nvec=nvec, bf16_head=True)
    g = ppo_cpp_amd.PPOHip(O, None if "nvec" in dist else nvec[0], list(HIDDEN), compute_dtype=dtype, **dist, **kw)
    set_weights("gaussian" if gauss else "multi", ref, g, 7, 2.0)
    g.set_bf16_queries(on)
    return ref, g


def inputs(head, n, seed=0):
    """(obs, noise, mask or None, valid given actions the policy did not draw); a mask forbids a category in every row and allows one per component"""
    nvec, rng, A, off = HEADS[head], np.random.RandomState(1000 * seed + n), sum(HEADS[head]), offsets(HEADS[head])
    obs = rng.uniform(-2, 2, (n, O)).astype(np.float32)
    if head.startswith("gauss"):
        return obs, rng.normal(size=(n, A)).astype(np.float32), None, rng.normal(size=(n, A)).astype(np.float32)
    mask = random_masks(rng, n, nvec, special=False) if head.endswith("_masked") else None
    if mask is not None:
        mask[mask.all(axis=1), 0] = 0.0                       # (component 0 has three categories or more: it still allows one)
    score = rng.uniform(size=(n, A)) + (0 if mask is None else mask)          # an allowed category scores above every forbidden one
    acts = np.stack([np.argmax(score[:, off[c]:off[c + 1]], axis=1) for c in range(len(nvec))], 1).astype(np.float32)
    return obs, np.clip(rng.uniform(size=(n, A)), 1e-6, 1 - 1e-6).astype(np.float32), mask, acts if head.startswith("multi") else acts[:, 0]


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("head", list(HEADS))
def test_the_steps_bits_and_float64_from_the_devices_own_head_sums(head, n):
    (ref, g), nvec, same, (obs, noise, mask, acts) = make(head), HEADS[head], np.testing.assert_array_equal, inputs(head, n)
    A, off = sum(nvec), offsets(nvec)
    a, v, nlp = g.step(obs, noise, mask=mask)
    same(np.stack(g.evaluate_actions(obs, a, mask)[:2]), np.stack([v, nlp]))          # the drawn action: the act model's bits
    (v2, nlp2, ent), par = g.evaluate_actions(obs, acts, mask), g.action_probability(obs, mask)      # given actions: float64 from the head's partial products [ranges][Rcap][128]
    parts = [g.debug_buffer(name).view(np.float32).reshape(4, -1, 128)[:, :n] for name in ("bf_head_pi", "bf_head_vf")]
    lg = R.head_sum_f32(parts[0])[:, :A].astype(np.float64); same(v2, R.head_sum_f32(parts[1])[:, 0])
    if head.startswith("gauss"):
        ls = ref.tensor("pi/logstd").astype(np.float64).reshape(-1)
        same(par[:, :A], g.act_deterministic(obs)); same(par[:, :A], lg.astype(np.float32))
        f = make(head, dtype=0, on=False)[1]                   # a PPO_F32 handle: the same expf; the setting changes no bit and no count there
        before, kc = f.evaluate_actions(obs, acts), f.kernel_counts()
        f.set_bf16_queries(True)
        same(np.stack(f.evaluate_actions(obs, acts)), np.stack(before)); same(par[:, A:], f.action_probability(obs)[:, A:])
        assert f.bf16_queries is True and f.kernel_counts() == kc
        close(par[:, A:], np.broadcast_to(np.exp(ls), (n, A)), "std")
        z = (acts.astype(np.float64) - lg) / np.exp(ls)
        rnlp, rent = 0.5 * (z * z).sum(axis=1) + 0.5 * np.log(2.0 * np.pi) * A + ls.sum(), np.full(n, (ls + HALF_LOG_2PIE).sum())
    else:
        want = np.concatenate([s[2] for s in E.head_stats(nvec, lg, mask)], axis=1)
        assert (np.abs(par.astype(np.float64) - want) <= prob_bound(want)).all()
        assert max(np.abs(par[:, off[c]:off[c + 1]].astype(np.float64).sum(axis=1) - 1.0).max() for c in range(len(nvec))) <= 2e-6
        rnlp, rent = E.neglogp_of(nvec, lg, acts, mask), E.entropy_of(nvec, lg, mask)
        assert mask is None or not par[mask == 0].view(np.uint32).any(), "a forbidden category's probability is exactly +0"
    close(nlp2, rnlp, "neglogp"); close(ent, rent, "entropy")


@pytest.mark.parametrize("head", ["gauss6", "cat6_masked", "multi"])
def test_rollout_evaluate_walks_a_rollout_larger_than_max_rows(head):
    _, g = make(head, max_rows=128)
    E_, T, same, cut = 50, 3, np.testing.assert_array_equal, lambda x: (None, None) if x is None else (x[:128], x[128:])      # 150 rows: chunks of 128 and 22
    g.set_action_masking(head.endswith("_masked"))
    g.rollout_alloc(E_, T); g.collect_synthetic(3, 0.99, 0.95)          # (no norm_init: normalisation off)
    obs, mask = g.rollout_get("obs").reshape(-1, O), None
    if head.endswith("_masked"):                               # an uploaded mask field, the actions re-drawn under it
        _, noise, mask, _ = inputs(head, E_ * T)
        drawn = [g.step(o, u, mask=m) for o, u, m in zip(cut(obs), cut(noise), cut(mask))]
        for field, x in (("masks", mask), ("actions", np.concatenate([d[0] for d in drawn])), ("neglogp", np.concatenate([d[2] for d in drawn]))):
            g.rollout_set(field, x.reshape(T, E_, -1) if field == "masks" else x.reshape(T, E_))
    out, acts = g.rollout_evaluate(), g.rollout_get("actions")
    same(out[0], g.rollout_get("values")); same(out[1], g.rollout_get("neglogp"))
    parts = [g.evaluate_actions(o, a, m) for o, a, m in zip(cut(obs), cut(acts.reshape((E_ * T,) + acts.shape[2:])), cut(mask))]
    same(np.stack(out).reshape(3, -1), np.concatenate([np.stack(p) for p in parts], axis=1))
    assert g.debug_buffer("bf_head_pi").size == 4 * 128 * 128, "the workspaces stay those of a step of max_rows"


@pytest.mark.parametrize("head", ["gauss70", "cat128_masked", "multi"])
def test_off_by_default_and_queries_between_steps_change_no_draw_and_no_count(head):
    obs, _, mask, acts = inputs(head, 130)
    runs = []
    for query in (False, True):
        g, out = make(head, on=False)[1], []
        kc = g.kernel_counts()
        for f in (lambda: g.evaluate_actions(obs, acts, mask), lambda: g.action_probability(obs, mask), lambda: g.rollout_evaluate()):
            with pytest.raises(Exception, match="PPO_BF16"):
                f()
        assert g.bf16_queries is False and g.kernel_counts() == kc and np.isfinite(g.value(obs)).all()
        g.set_bf16_queries(True)
        g.seed(11)
        for _ in range(3):
            if query:
                g.evaluate_actions(obs, acts, mask); g.action_probability(obs, mask)
            out.extend(x.reshape(-1) for x in g.step(obs, mask=mask)[::2])            # actions and neglogp
        runs.append((np.concatenate(out), g.kernel_counts(all_rows=True)))
    np.testing.assert_array_equal(runs[0][0], runs[1][0]); assert runs[0][1] == runs[1][1]
