"""The wide multi-binary head of the bf16 path: PPO_ACT_MULTI_BINARY | PPO_ACT_BF16_BINARY_HEAD | PPO_ACT_BF16_WIDE_BINARY_HEAD with compute_dtype PPO_BF16,
128 < act_dim <= 1024 (bf16_logits_kernel, bf16_value_head_kernel, bf16_{sample,loss,eval}_wide_binary_kernel<EPT>; include/ppo_hip.h).  The row kernels are fed the
DEVICE's own logits ("bf_head_pi", [1][Rcap][Ap] unsplit) and compared with float64 (bernoulli_ref.bern_stats) at tests/test_bf16_multi_binary.py's TOL.  A drawn bit
must equal u < p except where |u - p| < 1e-6 in float64, at most 0.1 % of the elements: the float64 reference alone (uniform u: about 2e-6) is held to that cap first.

    case     O   hidden     A     rows  what it hits
    A129     7   (40,)      129   24    EPT 4; first column past 127; a ragged quad; row stride not a multiple of 4; 127 padding columns
    A321     11  (136, 72)  321   130   EPT 8; dead rows in the last 16-row loss block and in the last 128-row GEMM tile
    A1024    5   (64,)      1024  20    EPT 16; no padding; the full LDS tile
"""
import ctypes
import inspect

import numpy as np
import pytest

from tests import bf16_ref as R
from tests import counter_draws_ref as D
from tests.bernoulli_ref import BernRef, bern_stats
from tests.bf16_cat_ref import synth_batch_from

gpu = pytest.mark.gpu
CR, LR, ENT, WIDE, NEAR, CAP = 0.16102319955825806, 0.000393141177482903, 0.01, 0x40000, 1e-6, 1e-3
TOL = dict(rtol=1e-4, atol=1e-5)                    # tests/test_bf16_multi_binary.py's
CASES = {"A129": (7, (40,), 129, 24), "A321": (11, (136, 72), 321, 130), "A1024": (5, (64,), 1024, 20)}
STEP, TRAIN, OLD = "bf16_step_sequence<wmbin>", "bf16_train_sequence<wmbin>", ("bf16_step_sequence<mbin>", "bf16_train_sequence<mbin>")
cases = pytest.mark.parametrize("case", list(CASES))


class Dev:
    def __init__(self, case, A=None, wide=True):
        import ppo_cpp_amd
        self.O, self.hidden, self.A, self.n = CASES[case]
        self.A = A or self.A
        self.ref = BernRef(self.O, self.A, self.hidden, ent_coef=ENT)
        self.ref.init_random(9, 1.0)
        self.g = ppo_cpp_amd.PPOHip(self.O, self.A, list(self.hidden), action_dist="multi_binary", compute_dtype=1, binary_bf16_head=True, binary_bf16_wide_head=wide, ent_coef=ENT)
        assert list(self.g.tensors) == [(n, s) for n, s in self.ref.specs], "the tensors of an fp32 multi-binary handle of the same act_dim"
        self.g.set_flat(self.ref.theta.astype(np.float32))
        self.lay = R.Layout(self.O, self.A, self.hidden)
        rng = np.random.RandomState(7)
        self.obs, self.u = rng.uniform(-1, 1, (self.n, self.O)).astype(np.float32), rng.uniform(size=(self.n, self.A)).astype(np.float32)

    def clear(self, u, logits):
        """the elements whose uniform is not within NEAR of p in float64; at most CAP of all may be left out"""
        ok = np.abs(np.asarray(u, np.float64) - bern_stats(logits)[0]) >= NEAR
        assert 1.0 - ok.mean() <= CAP
        return ok

    def logits_values(self):
        lg = self.g.debug_buffer("bf_head_pi").view(np.float32).reshape(-1, self.lay.Ap)
        vp = self.g.debug_buffer("bf_head_vf").view(np.float32).reshape(4, -1, 128)
        return lg[:self.n, :self.A].copy(), R.head_sum_f32(vp)[:self.n, 0]


@gpu
@cases
def test_stages_against_float64_from_the_devices_own_logits(case):
    d = Dev(case)
    g, lay, n, A, obs, u = d.g, d.lay, d.n, d.A, d.obs, d.u
    d.clear(u, d.ref.forward(obs)[0])                    # the float64 reference alone meets the cap
    a, v, nlp = g.step(obs, u)
    lg, v32 = d.logits_values()
    p, nlp1, nlp0, ent = bern_stats(lg)
    ok = d.clear(u, lg)
    np.testing.assert_array_equal(a[ok], (u < p)[ok].astype(np.float32)); assert set(np.unique(a)) <= {0.0, 1.0}
    np.testing.assert_array_equal(v, v32)
    np.testing.assert_allclose(nlp, np.where(a > 0, nlp1, nlp0).sum(1), **TOL)
    np.testing.assert_array_equal(g.act_deterministic(obs), (lg > 0).astype(np.float32))
    g.set_bf16_queries(True)
    prob = g.action_probability(obs)
    assert prob.shape == (n, A)
    np.testing.assert_allclose(prob, p, **TOL)
    np.testing.assert_allclose(g.evaluate_actions(obs, a)[2], ent.sum(1), **TOL)
    mb = synth_batch_from(obs, a, v, nlp, 3, CR)
    losses = g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    np.testing.assert_array_equal(d.logits_values()[0], lg)
    x, adv, old, R_, vo = [mb[k].astype(np.float64) for k in ("actions", "advs", "old_neglogp", "returns", "old_values")]
    cr = float(np.float32(CR))
    nlp64 = np.where(x > 0, nlp1, nlp0).sum(1)
    ratio = np.exp(old - nlp64)
    want = [np.maximum(-adv * ratio, -adv * np.clip(ratio, 1 - cr, 1 + cr)).mean(), 0.5 * np.maximum((v32 - R_) ** 2, (vo + np.clip(v32 - vo, -cr, cr) - R_) ** 2).mean(),
            ent.sum(1).mean(), 0.5 * ((nlp64 - old) ** 2).mean(), (np.abs(ratio - 1) > cr).mean()]
    print("\n%s losses %s float64 %s" % (case, losses, want))
    np.testing.assert_allclose(losses, want, **TOL)
    q = R.from_bits(g.debug_buffer("bf_dhead_pi").view(np.uint16)).reshape(-1, lay.Ap)[:R.ru(n, 128)]
    assert q[:n, :A].any() and not q[n:].view(np.uint32).any() and not q[:, A:].view(np.uint32).any(), "padding columns and dead rows are exactly +0"
    slots = g.debug_buffer("slots_pi").view(np.float32).reshape(-1, 2 * lay.Ap + 8)[:R.ru(n, 128) // 16]
    assert not slots[:, A:2 * lay.Ap].view(np.uint32).any(), "the padding's column sums and the aux slot words are zeros"
    assert g.kernel_count(STEP) == 2 and g.kernel_count(TRAIN) == 1 and not any(g.kernel_count(k) for k in OLD)
    g.close()


@gpu
@cases
def test_one_neglogp_in_three_places(case):
    """ppo_step's neglogp, ppo_evaluate_actions' on the drawn action and the train model's (approxkl == 0 on the step's own outputs) are the same bits; so is the value"""
    d = Dev(case)
    a, v, nlp = d.g.step(d.obs, d.u)
    d.g.set_bf16_queries(True)
    ev_v, ev_nlp, _ = d.g.evaluate_actions(d.obs, a)
    np.testing.assert_array_equal(ev_nlp, nlp); np.testing.assert_array_equal(ev_v, v)
    losses = d.g.train_step(LR, CR, d.obs, a, np.linspace(-1, 1, d.n).astype(np.float32), v + 0.3, nlp, v)
    assert losses[3] == 0.0 and losses[4] == 0.0 and np.isfinite(losses).all(), losses
    d.g.close()


@gpu
@pytest.mark.parametrize("case", ["A129", "A321"])
def test_gradient_of_one_train_step_against_the_float64_reference(case):
    """tests/test_bf16_wide_categorical.py's comparison of this name: cosine > 0.995 per tensor that carries more than 1e-3 of the norm, the global norm within 3 %;
    the pi/w columns and pi/b entries of the padding are exactly zero"""
    d = Dev(case)
    a, v, nlp, _ = d.ref.step(d.obs, d.u)
    mb = synth_batch_from(d.obs, a, v.astype(np.float32), nlp.astype(np.float32), 3, CR)
    args = (mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    _, ref_grad = d.ref.loss_grad(*args, CR)
    d.g.train_step(LR, CR, *args)
    grad, norm = d.g.last_grad()
    ref_norm = np.sqrt(ref_grad @ ref_grad)
    assert norm == pytest.approx(ref_norm, rel=3e-2)
    for name, (o, shape) in d.ref.offs.items():
        gt, rt = grad[o:o + int(np.prod(shape))], ref_grad[o:o + int(np.prod(shape))]
        if np.linalg.norm(rt) > 1e-3 * ref_norm:
            c = float(gt.astype(np.float64) @ rt / (np.linalg.norm(gt) * np.linalg.norm(rt)))
            assert c > 0.995, (name, c)
    padded = d.g.debug_buffer("grad").view(np.float32)
    assert d.lay.mat(padded, "pi/w")[:, :d.A].any() and not d.lay.mat(padded, "pi/w")[:, d.A:].any() and not d.lay.mat(padded, "pi/b")[0, d.A:].any()
    d.g.close()


@gpu
def test_on_device_draws_past_column_127():
    """noise = NULL: the bits are u < p built from counter_draws_ref's uniforms for j in [0, A)"""
    d = Dev("A321")
    u = D.counter_uniforms(D.seed_key(11), np.arange(d.n), 0, d.A).astype(np.float32)
    d.g.seed(11)
    a = d.g.step(d.obs)[0]
    lg = d.logits_values()[0]
    ok = d.clear(u, lg)
    np.testing.assert_array_equal(a[ok], (u < bern_stats(lg)[0])[ok].astype(np.float32))
    d.g.close()


def run_update(monkeypatch, switch):
    for s in ("PPO_HIP_NO_BF16_CHAIN", "PPO_HIP_NO_REDUCE_ADAM"):
        monkeypatch.delenv(s, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    E, T = 64, 8
    g = Dev("A321").g
    g.norm_init(E, 0.99); g.rollout_alloc(E, T)
    g.collect_synthetic(5, 0.99, 0.95)
    assert set(np.unique(g.rollout_get("actions"))) <= {0.0, 1.0}
    perms = np.stack([np.random.RandomState(2).permutation(E * T) for _ in range(2)]).astype(np.int32)
    out = [g.update(LR, CR, 2, 4, perms)[0]] + [g.get_flat(w) for w in range(3)]
    facts = g.debug_graph_nodes(), [g.kernel_count(k) for k in (STEP, TRAIN) + OLD], len(g.kernel_counts()), len(g.kernel_counts(all_rows=True))
    g.close()
    return out, facts


@gpu
def test_update_and_launch_forms(monkeypatch):
    """ppo_update on a synthetic rollout at A321 (E = 64, T = 8, 4 minibatches): finite rows, kernel nodes only, the new names count and the <mbin> ones stay 0, the frozen
    tables keep 60 / 62 rows; PPO_HIP_NO_BF16_CHAIN=1 and PPO_HIP_NO_REDUCE_ADAM=1 give the default form's bits"""
    want, (nodes, counts, rows, all_rows) = run_update(monkeypatch, None)
    assert np.isfinite(want[0]).all() and counts[0] > 0 and counts[1] == 8 and counts[2:] == [0, 0] and (rows, all_rows) == (60, 62), (counts, rows, all_rows)
    assert nodes is not None and nodes["kernel"] > 0 and nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    for switch in ("PPO_HIP_NO_BF16_CHAIN", "PPO_HIP_NO_REDUCE_ADAM"):
        for x, y in zip(want, run_update(monkeypatch, switch)[0]):
            np.testing.assert_array_equal(x, y, err_msg=switch)


def test_flag_contract_without_a_device():
    """parse_create answers before any HIP call: no GPU needed"""
    import os
    import ppo_cpp_amd
    from ppo_cpp_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "#define PPO_ACT_BF16_WIDE_BINARY_HEAD 0x40000\n" in open(os.path.join(root, "include", "ppo_hip.h")).read() and capi.ACT_BF16_WIDE_BINARY_HEAD == WIDE
    lib, cfg, h = ppo_cpp_amd.load_library(), capi.PPOConfig(), ctypes.c_void_p()

    def create(A, dist, dtype=1):
        lib.ppo_config_default(ctypes.byref(cfg), 7, A, 1, (ctypes.c_int32 * 1)(40))
        cfg.compute_dtype = dtype
        assert lib.ppo_create_ex(ctypes.byref(cfg), dist, ctypes.byref(h)) != 0
        return lib.ppo_last_error(None).decode()
    msg = create(1025, 3 | 0x8000 | WIDE)
    assert "PPO_ACT_BF16_WIDE_BINARY_HEAD" in msg and "1024" in msg and "1025" in msg, msg
    assert create(129, 3 | 0x8000) == "ppo_create_ex: PPO_ACT_BF16_BINARY_HEAD: the multi-binary head of the PPO_BF16 path holds at most 128 bits (got 129)"
    msg = create(6, 1 | WIDE, 0)
    assert "unknown action_dist" in msg and "PPO_ACT_BF16_WIDE_BINARY_HEAD" in msg, msg
    assert lib.ppo_create_multi_ex(ctypes.byref(cfg), (ctypes.c_int32 * 2)(3, 3), 2, WIDE, ctypes.byref(h)) != 0 and "unknown flag bit 0x40000" in lib.ppo_last_error(None).decode()
    with pytest.raises(ValueError, match="binary_bf16_wide_head belongs to action_dist='multi_binary'"):
        ppo_cpp_amd.PPOHip(7, 6, [40], action_dist="categorical", binary_bf16_wide_head=True)
    assert inspect.signature(ppo_cpp_amd.PPOHip.__init__).parameters["binary_bf16_wide_head"].default is False


@gpu
def test_narrow_flag_changes_nothing_and_refusals_leave_the_handle_usable(monkeypatch):
    from ppo_cpp_amd.capi import PPOHipError
    monkeypatch.setenv("PPO_RCCL_LIBRARY", "/nonexistent/no_collective_library.so")
    runs = []
    for wide in (False, True):                           # act_dim <= 128: the flag changes nothing -- same bits, same variant counts
        d = Dev("A129", A=70, wide=wide)
        assert d.g.binary_bf16_wide_head is wide
        runs.append(list(d.g.step(d.obs, d.u)) + [np.array(sorted(d.g.kernel_variants().items()), dtype=object)])
        d.g.close()
    for x, y in zip(*runs):
        np.testing.assert_array_equal(x, y)
    d = Dev("A129")
    g, obs = d.g, d.obs
    want = g.act_deterministic(obs)
    for call, text in ((lambda: g.step(obs, mask=np.ones((d.n, d.A), np.float32)), "action masks need a categorical"),
                       (lambda: g.set_target_kl(0.01), "ppo_set_target_kl: not supported on a PPO_BF16 handle"),
                       (lambda: g.dist_init(1, 0, bytes(128)), "data parallel is not supported for a multi-binary PPO_BF16 handle created with PPO_ACT_BF16_BINARY_HEAD")):
        with pytest.raises(PPOHipError, match=text):
            call()
        np.testing.assert_array_equal(g.act_deterministic(obs), want)
        assert np.isfinite(g.step(obs)[2]).all()
    g.close()
