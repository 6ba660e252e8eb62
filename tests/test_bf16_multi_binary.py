"""The multi-binary head of the bf16 matrix-core path: PPO_ACT_MULTI_BINARY | PPO_ACT_BF16_BINARY_HEAD with compute_dtype PPO_BF16 (include/ppo_hip.h).  The GEMMs
around the head are every PPO_BF16 handle's (tests/test_bf16_stages.py); here bf16_sample_kernel / bf16_loss_kernel / bf16_eval_kernel<mbin> are fed the DEVICE's own
logits -- the head GEMM's partial products ("bf_head_pi") added in range order -- and compared with float64 (bernoulli_ref.bern_stats) at tests/test_multi_binary.py's
tolerances; the bf16 d logits under tests/bf16_ref.py's rules (1) and (2) with E and the share cap taken from the fp32 emulation (bernoulli_ref.emulate_f32's pieces).
Weights BernRef.init_random(9, pi_gain=1.0), observations and uniforms RandomState(7).  OBSERVED on an MI355X:
    case                   emulation |err| max   E (10 x; floor 2^-22 |y|)   emulation share   device share q != rne(y)
    A6_ragged_dead_rows    4.49e-9               4.49e-8                     0 of 780          0 of 780
    A70_second_element     6.56e-8               6.56e-7                     3.35e-4           1.12e-4 of 8960
    A128_no_padding        1.18e-7               1.18e-6                     8.54e-4           4.88e-4 of 8192
    A1_one_bit             2.66e-9               2.66e-8                     0 of 64           0 of 64
    loss terms against float64: 7 digits (entropy 48.174187 against 48.17418872 at A70); update rows beside the fp32 handle: entropy within 4e-7 relative, vf_loss 4e-4
"""
import ctypes as C

import numpy as np
import pytest

from tests import bf16_ref as R
from tests.bernoulli_ref import BernRef, bern_stats, emulate_f32
from tests.bf16_cat_ref import synth_batch_from

gpu = pytest.mark.gpu
CR, LR, GAMMA, LAM, ENT, BF16, FLAG = 0.16102319955825806, 0.000393141177482903, 0.99, 0.95, 0.01, 1, 0x8000
TOL = dict(rtol=1e-4, atol=1e-5)                    # tests/test_multi_binary.py's
# (hidden, O, A, n): the smallest shapes that reach each way the three kernels can go wrong; CHAIN: chained launches, the update case only
CASES = {"A6_ragged_dead_rows": ((256, 128), 18, 6, 130), "A70_second_element": ((1280,), 18, 70, 128), "A128_no_padding": ((128,), 7, 128, 64), "A1_one_bit": ((128,), 7, 1, 64)}
CHAIN = ((512, 512), 64, 18, 2048)


def test_flag_contract_without_a_device():
    import torch
    import ppo_cpp_amd
    from ppo_cpp_amd.capi import PPOConfig
    lib, cfg, h = ppo_cpp_amd.load_library(), PPOConfig(), C.c_void_p()

    def create_ex(word, act_dim=18, dtype=0):
        lib.ppo_config_default(C.byref(cfg), 18, act_dim, 2, (C.c_int32 * 2)(64, 64))
        cfg.compute_dtype = dtype
        rc = lib.ppo_create_ex(C.byref(cfg), word, C.byref(h))
        if rc == 0:
            lib.ppo_destroy(h)
        return lib.ppo_last_error(None).decode() if rc else ""
    msg = create_ex(3 | FLAG)
    assert "unknown" not in msg and (torch.cuda.is_available() or "no HIP device" in msg), msg
    msg = create_ex(3 | FLAG, 129, BF16)
    assert "PPO_ACT_BF16_BINARY_HEAD" in msg and "128" in msg and "129" in msg, msg
    for word in (1 | FLAG, 0 | FLAG):
        msg = create_ex(word)
        assert "unknown action_dist" in msg and "PPO_ACT_BF16_BINARY_HEAD" in msg, msg
    assert lib.ppo_create_multi_ex(C.byref(cfg), (C.c_int32 * 2)(9, 9), 2, FLAG, C.byref(h)) != 0 and "unknown flag bit 0x8000" in lib.ppo_last_error(None).decode()
    assert create_ex(3, 18, BF16) == "ppo_create_ex: PPO_ACT_MULTI_BINARY with compute_dtype PPO_BF16 is not supported (the multi-binary head runs on the PPO_F32 path)"
    with pytest.raises(ValueError, match="binary_bf16_head belongs to action_dist='multi_binary'"):
        ppo_cpp_amd.PPOHip(18, 18, [64, 64], action_dist="categorical", binary_bf16_head=True)


class Dev:
    def __init__(self, hidden, O, A, dtype=BF16, flag=True, pi_gain=1.0):
        import ppo_cpp_amd
        self.ref = BernRef(O, A, hidden, ent_coef=ENT)
        self.ref.init_random(9, pi_gain)
        self.g = ppo_cpp_amd.PPOHip(O, A, list(hidden), action_dist="multi_binary", compute_dtype=dtype, binary_bf16_head=flag, ent_coef=ENT)
        assert list(self.g.tensors) == [(n, s) for n, s in self.ref.specs]
        self.g.set_flat(self.ref.theta.astype(np.float32))
        self.A, self.lay = A, R.Layout(O, A, hidden)

    def logits_values(self, n):
        parts = [self.g.debug_buffer(k).view(np.float32).reshape(4, -1, self.lay.Ap)[:, :R.ru(n, 128)] for k in ("bf_head_pi", "bf_head_vf")]
        return R.head_sum_f32(parts[0])[:n, :self.A], R.head_sum_f32(parts[1])[:n, 0]

    def inputs(self, O, n):
        """observations, explicit uniforms kept 2e-4 clear of the device's own p (tests/test_multi_binary.py's rule), the logits a first step leaves, p in float64"""
        rng = np.random.RandomState(7)
        obs, u = rng.uniform(-1, 1, (n, O)).astype(np.float32), rng.uniform(size=(n, self.A)).astype(np.float32)
        self.g.step(obs)
        lg = self.logits_values(n)[0]
        p = bern_stats(lg)[0]
        return obs, np.where(np.abs(u - p) < 1e-4, np.where(p > 0.5, p - 2e-4, p + 2e-4), u).astype(np.float32), lg, p


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_step_and_train_step_from_the_devices_own_logits(case):
    hidden, O, A, n = CASES[case]
    d = Dev(hidden, O, A)
    g, lay = d.g, d.lay
    obs, u, lg0, p = d.inputs(O, n)
    a, v, nlp = g.step(obs, u)
    lg, v32 = d.logits_values(n)
    np.testing.assert_array_equal(lg, lg0, err_msg="the same observations give the same logits")
    np.testing.assert_array_equal(a, (u < p).astype(np.float32)); np.testing.assert_array_equal(v, v32)
    np.testing.assert_array_equal(g.act_deterministic(obs), (lg > 0).astype(np.float32))
    np.testing.assert_allclose(nlp, np.where(a > 0, *bern_stats(lg)[1:3]).sum(1), **TOL)
    off = lay.t["pi/logstd"][0]
    before = [g.debug_buffer(k)[off:off + 256].copy() for k in ("theta", "adam_m", "adam_v")]
    mb = synth_batch_from(obs, a, v, nlp, 3, CR)
    assert (mb["advs"] > 0).any() and (mb["advs"] < 0).any()
    losses = g.train_step(LR, CR, mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    lg, v32 = d.logits_values(n)
    x, adv, old = [mb[k].astype(np.float64) for k in ("actions", "advs", "old_neglogp")]
    cr, gn = float(np.float32(CR)), 1.0 / n

    def dlogits(f, p_, nlp_rows, pq):                 # ppo_head.hpp's surrogate_row / surrogate_d_nlp / bern_grad_elem in the arithmetic of type f
        ratio = np.exp((old.astype(f) - nlp_rows).astype(f)).astype(f)
        rmin = np.minimum(ratio, f(1 + cr)); rclip = np.maximum(rmin, f(1 - cr))
        m1, m2 = (-adv.astype(f) * ratio).astype(f), (-adv.astype(f) * rclip).astype(f)
        d_ratio = np.where((m1 >= m2) | ((rmin >= f(1 - cr)) & (ratio <= f(1 + cr))), (-adv.astype(f) * f(gn)).astype(f), f(0))
        d_nlp = (-(d_ratio * ratio)).astype(f)
        return (d_nlp[:, None] * (p_ - x.astype(f)) + (f(ENT) * f(gn)) * (lg.astype(f) * pq)).astype(f), ratio, np.maximum(m1, m2)
    p64, nlp1, nlp0, ent = bern_stats(lg)
    nlp64 = np.where(x > 0, nlp1, nlp0).sum(1)
    y, ratio, pg_rows = dlogits(np.float64, p64, nlp64, p64 * (1 - p64))
    p32, _, nlp32, _, pq32 = emulate_f32(lg, x=x.astype(np.float32))
    emu = dlogits(np.float32, p32, nlp32, pq32)[0]
    err, share_ref = float(np.abs(emu - y).max()), R.mismatch_share(R.rne_bf16(emu), y)
    E = np.maximum(10 * err, 2.0 ** -22 * np.abs(y))
    q = R.from_bits(g.debug_buffer("bf_dhead_pi").view(np.uint16)).reshape(-1, lay.Ap)[:R.ru(n, 128)]
    print("\n%s d logits: emulation |err| max %.3g, E %.3g, emulation share %.3g, device share %.3g of %d" % (case, err, 10 * err, share_ref, R.mismatch_share(q[:n, :A], y), n * A))
    R.check_bf16(case + " d logits", q[:n, :A], y, E, share_ref)
    assert not q[n:].view(np.uint32).any() and not q[:, A:].view(np.uint32).any(), "padding columns and dead rows are exactly +0"
    slots = g.debug_buffer("slots_pi").view(np.float32).reshape(-1, 2 * lay.Ap + 8)[:R.ru(n, 128) // 16]
    assert not slots[:, lay.Ap:2 * lay.Ap].view(np.uint32).any(), "the aux (d logstd) slot words are zeros"
    ob = d.ref.offs["pi/b"][0]
    R.check_f32(case + " grad pi/b", g.last_grad()[0][ob:ob + A], *R.column_sums(y, E, n))
    R_, vo = mb["returns"].astype(np.float64), mb["old_values"].astype(np.float64)
    want = [pg_rows.mean(), 0.5 * np.maximum((v32 - R_) ** 2, (vo + np.clip(v32 - vo, -cr, cr) - R_) ** 2).mean(), ent.sum(1).mean(), 0.5 * ((nlp64 - old) ** 2).mean()]
    print("%s losses %s float64 %s" % (case, losses, want))
    np.testing.assert_allclose(losses[:4], want, **TOL)
    assert abs(losses[4] - (np.abs(ratio - 1) > cr).mean()) <= 1.0 / n + 1e-7
    for k, b in zip(("theta", "adam_m", "adam_v"), before):
        np.testing.assert_array_equal(g.debug_buffer(k)[off:off + 256], b, err_msg="padded logstd region of " + k)
    kv = g.kernel_variants()
    assert kv["bf16_step_sequence<mbin>"] == 3 and kv["bf16_train_sequence<mbin>"] == 1 and kv["bf16_step_sequence"] == 0 and kv["bf16_train_sequence"] == 0, kv
    g.close()


@gpu
def test_bitwise_properties():
    hidden, O, A, n = CASES["A70_second_element"]
    runs = []
    for rep in range(2):
        d = Dev(hidden, O, A)
        obs, u, lg, p = d.inputs(O, n)
        d.g.seed(5)
        seeded = d.g.step(obs)
        a, v, nlp = d.g.step(obs, u)
        d.g.set_bf16_queries(True)
        ev, enlp, eent = d.g.evaluate_actions(obs, a)
        np.testing.assert_array_equal(ev, v); np.testing.assert_array_equal(enlp, nlp)
        np.testing.assert_allclose(eent, bern_stats(lg)[3].sum(1), **TOL)
        prob = d.g.action_probability(obs)
        assert prob.shape == (n, A) and prob.min() >= 0 and prob.max() <= 1
        np.testing.assert_allclose(prob, p, rtol=0, atol=1e-6)
        adv = np.random.RandomState(1).normal(size=n).astype(np.float32)
        losses = d.g.train_step(LR, CR, obs, a, adv, (v + adv).astype(np.float32), nlp, v)          # what ppo_step just returned, weights unchanged
        assert losses[3] == 0.0 and losses[4] == 0.0 and np.isfinite(losses).all(), losses
        runs.append([a, v, nlp, losses, d.g.get_flat(0)] + list(seeded))
        d.g.close()
    hidden, O, A, n = CASES["A6_ragged_dead_rows"]      # PPO_F32 with the flag against without (the generic fp32 family cannot hold a 1280-wide layer)
    for flag in (False, True):
        d = Dev(hidden, O, A, dtype=0, flag=flag)
        d.g.seed(5)
        runs.append(list(d.g.step(np.random.RandomState(7).uniform(-1, 1, (n, O)).astype(np.float32))) + [np.array(sorted(d.g.kernel_variants().items()), dtype=object)])
        d.g.close()
    for one, other in (runs[:2], runs[2:]):
        for x, y in zip(one, other):
            np.testing.assert_array_equal(x, y)


@gpu
def test_update_beside_the_fp32_multi_binary_handle():
    """collect_synthetic + two updates (the second a graph replay) under tests/test_bf16_path.py's end-to-end criteria; the policy head starts at its usual gain 0.01"""
    hidden, O, A, n = CHAIN
    E, T, nmb, epochs = 64, 32, 1, 2
    db, df = Dev(hidden, O, A, pi_gain=0.01), Dev(hidden, O, A, dtype=0, flag=False, pi_gain=0.01)
    gb, gf = db.g, df.g
    perms = np.stack([np.random.RandomState(9).permutation(E * T) for _ in range(epochs)]).astype(np.int32)
    rows = []
    for g in (gb, gf):
        g.seed(11); g.norm_init(E, GAMMA); g.rollout_alloc(E, T)
        g.collect_synthetic(1234, GAMMA, LAM)
        assert set(np.unique(g.rollout_get("actions"))) <= {0.0, 1.0}
        rows.append(np.concatenate([g.update(LR, CR, epochs, nmb, perms)[0] for _ in range(2)]))
    np.testing.assert_allclose(gb.rollout_get("values"), gf.rollout_get("values"), rtol=3e-2, atol=3e-2)
    np.testing.assert_allclose(gb.rollout_get("returns"), gf.rollout_get("returns"), rtol=3e-2, atol=5e-2)
    rb, rf = rows
    print("\nbf16 rows\n%s\nfp32 rows\n%s" % (rb, rf))
    for k, kw in enumerate((dict(atol=1e-2), dict(rtol=2e-2), dict(rtol=1e-4), dict(rtol=1e-2, atol=2e-3), dict(atol=0.06))):      # pg, vf, entropy, approxkl, clipfrac
        np.testing.assert_allclose(rb[:, k], rf[:, k], err_msg="loss column %d" % k, **kw)
    da, dc = [(g.get_flat(0) - db.ref.theta.astype(np.float32)).astype(np.float64) for g in (gb, gf)]
    assert da @ dc / (np.linalg.norm(da) * np.linalg.norm(dc)) > 0.9
    nodes = gb.debug_graph_nodes()
    assert nodes is not None and nodes["kernel"] > 0 and nodes["memset"] == 0 and nodes["memcpy"] == 0 and nodes["other"] == 0, nodes
    kv = gb.kernel_variants()
    assert kv["bf16_step_sequence<mbin>"] > 0 and gb.kernel_count("bf16_train_sequence<mbin>") == epochs * nmb, kv      # (one capture; the replay counts nothing)
    assert kv["bf16_step_sequence"] == 0 and kv["bf16_train_sequence"] == 0 and len(gb.kernel_counts()) == 60
    gb.close(); gf.close()


@gpu
def test_refusals_leave_the_handle_usable(monkeypatch):
    from ppo_cpp_amd.capi import PPOHipError
    monkeypatch.setenv("PPO_RCCL_LIBRARY", "/nonexistent/no_collective_library.so")
    hidden, O, A, n = CASES["A6_ragged_dead_rows"]
    g = Dev(hidden, O, A).g
    obs = np.random.RandomState(7).uniform(-1, 1, (n, O)).astype(np.float32)
    want = g.act_deterministic(obs)
    for call, text in ((lambda: g.step(obs, mask=np.ones((n, A), np.float32)), "action masks need a categorical"),
                       (lambda: g.set_target_kl(0.01), "ppo_set_target_kl: not supported on a PPO_BF16 handle"),
                       (lambda: g.dist_init(1, 0, bytes(128)), "data parallel is not supported for a multi-binary PPO_BF16 handle created with PPO_ACT_BF16_BINARY_HEAD"),
                       (lambda: g.evaluate_actions(obs, want), "not supported on a PPO_BF16 handle")):
        with pytest.raises(PPOHipError, match=text):
            call()
        np.testing.assert_array_equal(g.act_deterministic(obs), want)
        assert np.isfinite(g.step(obs)[2]).all()
    g.close()
